// ef_binarize.hip — every kernel of EarlyFusion's binarisation, and their launchers.
//
// The rule (csm_to_binary; ef_select.hpp holds it once): the nn = count(kappa, n) least cells of a
// line of n become 1, ties to the lowest index. Rows of the float32 CSMs: least; rows of early SNF's
// float64 cross block: largest. The mutual rule (Tralie 2017; the definition: include/acoss_hip.h,
// "mutual") ANDs the same select down the columns into what the rows left.
//
// The masks are a pair's bit planes: u16 words of 16 rows of ONE column, Wb[plane * wplane + g * ld
// + c], bit r = row 16 g + r (the Smith-Waterman input). A row kernel writes fresh words; the column
// pass clears bits in them: C(i, j) stays iff fewer than nn_c = count(kappa, M) cells of column j
// come before (i, j) in (value, row) order. Each kernel is load (keys into registers), select
// (ef_select.hpp) and emit (bits into words); by the batch's pitch ld, a multiple of 4:
//
//   ld       rows (ef_launch_rowbin)                       columns (ef_launch_colpass)
//   <= 64    k_ef_binarize_lanes: a wave per (pair,        k_ef_colpass_lanes: a wave per (pair,
//            matrix), a row per lane, knock64; where       matrix), a column per lane, knock64
//            count(kappa, 64) > 8, or ACOSS_EF_LANEBIN=0,  (ACOSS_EF_COLLANES=0: the next class)
//            k_ef_binarize_small: a block per (pair,
//            matrix), a wave per row
//   <= 512   k_ef_binarize: a block per 16 rows, a wave    k_ef_colpass_wave<8>: a block per 32
//            per row, 8 key registers per lane             columns, a wave per column, 8 key registers
//   <= 1024  ... 16 key registers                          k_ef_colpass_wave<16> (ACOSS_EF_COLWAVE=0:
//                                                          the next class for both)
//   above    ... the bisection, the row read per pass      k_ef_colpass<float>: a lane per column
// A wave per row takes rows of at most 64 columns with nn <= kKnockMax by wave-minimum rounds
// (ef_binarize_row_knock), every other row by the halves of wave_line_select or of its _stream form.
// Early SNF: k_efs_binarize (rank count, any ld) and k_ef_colpass<double>.
// Every loop bound is wave-uniform (M, N, nn, the digit count); a block leaves as a whole.
// acoss_binarize_mutual runs the row launch and the column pass over a batch of caller matrices;
// only the copy-in, the bank and the unpack kernels are its own.
#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "common.hpp"
#include "ef_internal.hpp"
#include "ef_select.hpp"

namespace acoss {
namespace {

constexpr int kBinRegs = 16;  // row keys per lane kept in registers by k_ef_binarize (N <= 1024)

// ---- rows ------------------------------------------------------------------------------------------
// The nn smallest of one row -> `bit` of bits[column] (LDS words the block zeroed), by one wave.
template <int KB>  // keys per lane held in registers (rows of up to 64 * KB columns)
__device__ __forceinline__ void ef_binarize_row(const float* __restrict__ x, int N, double kappa, int lane,
                                                unsigned* bits, unsigned bit, unsigned* hist) {
  if (kappa == 0.0) {
    for (int c = lane; c < N; c += 64) atomicOr(&bits[c], bit);
    return;
  }
  const int nn = ef_count(kappa, N);
  if (nn <= 0) return;
  const int per = (N + 63) / 64;
  const int c0 = lane * per, c1 = min(N, c0 + per);
  // The two halves of each select, the branches meeting in between, not wave_line_select in one arm
  // and wave_line_select_stream in the other: there the compiler keeps the KB guards of the range
  // bound in scalar register pairs across radix_kth for the keep loop, and k_ef_binarize goes from
  // 79 to 106 SGPRs and from 8 to 7 waves per SIMD (profiles/ef_binarize/README.md)
  const bool inreg = per <= KB;
  auto at = [&](int k) { return fkey_f32(x[k]); };
  unsigned kr[KB], kth;
  if (inreg) {  // the row's keys in registers: one pass over memory
#pragma unroll
    for (int q = 0; q < KB; ++q) kr[q] = (q < per && c0 + q < c1) ? at(c0 + q) : 0xffffffffu;
    kth = wave_line_kth(kr, per, c0, c1, nn, lane, hist);
  } else {
    kth = wave_stream_kth(at, c0, c1, nn);
  }
  auto put = [&](int c, bool v) {
    if (v) atomicOr(&bits[c], bit);
  };
  if (inreg)
    wave_line_keep(kr, kth, per, c0, c1, nn, [&](int q, bool v) { put(c0 + q, v); });
  else
    wave_stream_keep(at, kth, c0, c1, nn, put);
}

// Rows of at most 64 columns (one key per lane) with a small nn (Da-TACOS beat blocks: N ~ 14..47,
// nn = round(kappa N) ~ 1..5): nn rounds of (wave minimum of the remaining keys, the lowest lane
// holding it leaves and sets its bit). Each round takes the least remaining key and, among equal
// keys, the lowest column, so the nn lanes taken are exactly csm_to_binary's nn smallest with ties
// to the lowest column -- the radix select's answer at a fraction of its passes.
__device__ __forceinline__ void ef_binarize_row_knock(const float* __restrict__ x, int N, int nn, int lane,
                                                      unsigned* bits, unsigned bit) {
  unsigned k = lane < N ? fkey_f32(x[lane]) : 0xffffffffu;
  bool alive = lane < N;
  for (int t = 0; t < nn; ++t) {  // wave-uniform
    const unsigned m = wave_min_u32(alive ? k : 0xffffffffu);
    const int src = __builtin_ctzll(__ballot(alive && k == m));
    if (lane == src) {
      alive = false;
      atomicOr(&bits[lane], bit);
    }
  }
}
constexpr int kKnockMax = 16;  // largest nn taken by ef_binarize_row_knock

// A block of 16 waves takes 16 rows (one wave per row) and writes them as one row of u16 bit words
// (bit r = row 16g + r) in LDS, then to the pair's bit plane. blockIdx.z = CSM plane, written to
// bit plane z + plane0 of the pair (plane stride = wplane words, 4 planes per pair).
__global__ __launch_bounds__(1024) void k_ef_binarize(const float* __restrict__ C, int64_t mat_stride, int ld,
                                                      EfPairs E, double kappa, uint16_t* __restrict__ Wb,
                                                      int64_t wplane, int plane0) {
  extern __shared__ unsigned bits[];
  __shared__ __attribute__((aligned(16))) unsigned s_hist[16][256 + 64];  // radix_kth, one per wave
  const int p = blockIdx.y, m = blockIdx.z, g = blockIdx.x;
  int a, b, M, N;
  pair_dims(E, p, &a, &b, &M, &N);
  if (16 * g >= M) return;  // whole block: no barrier skipped by part of it
  for (int c = threadIdx.x; c < N; c += 1024) bits[c] = 0;
  __syncthreads();
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int row = 16 * g + w;
  if (row < M) {
    const float* xr = C + m * mat_stride + (size_t)p * ld * ld + (size_t)row * ld;
    const int nn = ef_count(kappa, N);
    if (N <= 64 && kappa != 0.0 && nn <= kKnockMax) {
      if (nn > 0) ef_binarize_row_knock(xr, N, nn, lane, bits, 1u << w);
    } else if (N <= 64 * 8)  // EarlyFusion's ~450-block tracks: 8 key registers halve the count passes
      ef_binarize_row<8>(xr, N, kappa, lane, bits, 1u << w, s_hist[w]);
    else
      ef_binarize_row<kBinRegs>(xr, N, kappa, lane, bits, 1u << w, s_hist[w]);
  }
  __syncthreads();
  uint16_t* o = Wb + ((size_t)p * 4 + plane0 + m) * wplane + (size_t)g * ld;
  for (int c = threadIdx.x; c < N; c += 1024) o[c] = (uint16_t)bits[c];
}

// k_ef_binarize for batches whose tracks all have at most 64 blocks and a small nn (Da-TACOS beat
// blocks, kappa = 0.1: nn = 1..6): ONE WAVE per (pair, matrix), lane r = row r. The lane loads its
// row's keys into registers (16-byte loads) and takes its nn least (knock64); a ballot per column
// then gives lane c its column's 64-bit row mask, which it writes as the u16 words of the SW bit
// plane. No LDS, no barrier, no cross-lane reduction per round (k_ef_binarize_small spent 4 waves,
// two block barriers and a 6-stage wave minimum per round and row).
__global__ __launch_bounds__(256) void k_ef_binarize_lanes(const float* __restrict__ C, int64_t mat_stride, int ld,
                                                           EfPairs E, double kappa, uint16_t* __restrict__ Wb,
                                                           int64_t wplane, int plane0, int nplanes, int n_units) {
  const int unit = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (unit >= n_units) return;
  const int p = unit / nplanes, m = unit - p * nplanes;
  int a, b, M, N;
  pair_dims(E, p, &a, &b, &M, &N);
  const int lane = threadIdx.x & 63;
  const int nn = ef_count(kappa, N);
  unsigned long long sel = 0ull;  // this lane's row: its selected columns
  if (kappa == 0.0) {
    sel = N >= 64 ? ~0ull : ((1ull << N) - 1ull);
  } else if (nn > 0) {
    const float* xr = C + m * mat_stride + (size_t)p * ld * ld + (size_t)min(lane, M - 1) * ld;
    unsigned key[64];
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      if (4 * q < N) {  // wave-uniform; ld is a multiple of 4, so the 16-byte load stays in the row
        const f32x4e v = *reinterpret_cast<const f32x4e*>(xr + 4 * q);
#pragma unroll
        for (int u = 0; u < 4; ++u) key[4 * q + u] = 4 * q + u < N ? fkey_f32(v[u]) : 0xffffffffu;
      } else {
#pragma unroll
        for (int u = 0; u < 4; ++u) key[4 * q + u] = 0xffffffffu;
      }
    }
    sel = knock64(key, N, nn);
  }
  const unsigned long long rows = M >= 64 ? ~0ull : ((1ull << M) - 1ull);
  unsigned long long colbits = 0ull;
#pragma unroll
  for (int c = 0; c < 64; ++c) {
    if (c < N) {
      const unsigned long long bcol = __ballot((sel >> c) & 1ull) & rows;
      colbits = lane == c ? bcol : colbits;
    }
  }
  const int ng = (M + 15) / 16;
  uint16_t* o = Wb + ((size_t)p * 4 + plane0 + m) * wplane;
  if (lane < N)
    for (int g = 0; g < ng; ++g) o[(size_t)g * ld + lane] = (uint16_t)(colbits >> (16 * g));
}

// k_ef_binarize for batches whose tracks all have at most 64 blocks (Da-TACOS beat blocks): ONE
// 256-thread block per (pair, matrix) instead of a 1024-thread block per 16 rows; wave w takes
// rows w, w + 4, ... with the same per-row selects as k_ef_binarize, into LDS words of 16 rows.
__global__ __launch_bounds__(256) void k_ef_binarize_small(const float* __restrict__ C, int64_t mat_stride, int ld,
                                                           EfPairs E, double kappa, uint16_t* __restrict__ Wb,
                                                           int64_t wplane, int plane0) {
  __shared__ unsigned bits[4][64];
  __shared__ __attribute__((aligned(16))) unsigned s_hist[4][256 + 64];  // radix_kth, one per wave
  const int p = blockIdx.x, m = blockIdx.y;
  int a, b, M, N;
  pair_dims(E, p, &a, &b, &M, &N);
  for (int e = threadIdx.x; e < 4 * 64; e += 256) bits[e >> 6][e & 63] = 0u;
  __syncthreads();
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int nn = ef_count(kappa, N);
  for (int row = w; row < M; row += 4) {
    const float* xr = C + m * mat_stride + (size_t)p * ld * ld + (size_t)row * ld;
    unsigned* brow = bits[row >> 4];
    const unsigned bit = 1u << (row & 15);
    if (kappa != 0.0 && nn <= kKnockMax) {
      if (nn > 0) ef_binarize_row_knock(xr, N, nn, lane, brow, bit);
    } else {
      ef_binarize_row<8>(xr, N, kappa, lane, brow, bit, s_hist[w]);
    }
  }
  __syncthreads();
  const int ng = (M + 15) / 16;
  uint16_t* o = Wb + ((size_t)p * 4 + plane0 + m) * wplane;
  for (int e = threadIdx.x; e < ng * 64; e += 256) {
    const int g = e >> 6, c = e & 63;
    if (c < N) o[(size_t)g * ld + c] = (uint16_t)bits[g][c];
  }
}

// Early SNF: the nn LARGEST of every row of cross -> 1, ties to the lowest column (csm_to_binary of
// exp(-cross)): column c is taken when fewer than nn columns come before it in that order. A block
// takes 16 rows (4 waves, 4 rows each, a row at a time in the wave's LDS line) and writes them as
// one row of u16 words of the pair's bit plane. A pair the reference cannot fuse gets an empty plane.
__global__ __launch_bounds__(256) void k_efs_binarize(const double* __restrict__ cr, int ld, EfPairs E, int K,
                                                      double kappa, uint16_t* __restrict__ Wb, int64_t wplane) {
  extern __shared__ double s_line[];  // 4 lines of ld doubles, then ld u32 bit words
  const int p = blockIdx.y, g = blockIdx.x;
  int a, b, M, N, k1, k2;
  pair_dims(E, p, &a, &b, &M, &N);
  if (16 * g >= M) return;  // the whole block
  unsigned* bits = reinterpret_cast<unsigned*>(s_line + 4 * ld);
  for (int c = threadIdx.x; c < N; c += 256) bits[c] = 0u;
  __syncthreads();
  const bool ok = snf_split(M, N, K, &k1, &k2);
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int nn = ef_count(kappa, N);
  double* line = s_line + w * ld;
  for (int q = 0; q < 4 && ok; ++q) {
    const int rr = w + 4 * q, row = 16 * g + rr;
    if (row >= M) break;  // wave-uniform
    const double* x = cr + (size_t)p * ld * ld + (size_t)row * ld;
    __builtin_amdgcn_wave_barrier();
    for (int c = lane; c < N; c += 64) line[c] = x[c];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    for (int c = lane; c < N; c += 64) {
      bool take = kappa == 0.0;
      if (!take) {
        const double v = line[c];
        int before = 0;
        for (int j = 0; j < N; ++j) {
          const double u = line[j];
          before += (u > v || (u == v && j < c)) ? 1 : 0;
        }
        take = before < nn;
      }
      if (take) atomicOr(&bits[c], 1u << rr);
    }
  }
  __syncthreads();
  uint16_t* o = Wb + (size_t)p * wplane + (size_t)g * ld;
  for (int c = threadIdx.x; c < N; c += 256) o[c] = (uint16_t)bits[c];
}

// ---- columns: a lane owns a column, so it clears whole words, and adjacent lanes read adjacent
// elements of a matrix row ---------------------------------------------------------------------------
constexpr int kColBins = 16;  // 4-bit digits

// Any ld, and the float64 / largest form of early SNF: a wave per 64 columns of a (pair, matrix);
// lane-private radix select, 4-bit digits from the top, each digit from one pass down the column
// into the lane's own 16 LDS bins, then one pass that rebuilds the words.
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
// rows l * per .. l * per + per - 1 of the column (per = ceil(M / 64) <= KB; one strided load each)
// and the wave selects (wave_line_select). The kept rows go to LDS words of 16 rows (a lane's rows
// span at most two), and the block ANDs them into the plane. A block takes 32 adjacent columns, so
// the 128-byte lines its strided loads touch are fetched once and shared by its waves.
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
    const int g0 = r0 >> 4;
    unsigned wlo = 0u, whi = 0u;  // the lane's rows in word g0 and in word g0 + 1
    wave_line_select<KB>(kr, per, r0, r1, nn, lane, s_hist[w], [&](int q, bool v) {
      const unsigned bit = v ? 1u << ((r0 + q) & 15) : 0u;
      wlo |= ((r0 + q) >> 4) == g0 ? bit : 0u;
      whi |= ((r0 + q) >> 4) == g0 ? 0u : bit;
    });
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
// consecutive floats of a row), takes its nn_c least (knock64), and the 64-bit row mask is ANDed
// into the column's words.
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
    sel = knock64(key, M, nn);
  }
  const int ng = (M + 15) / 16;
  uint16_t* o = Wb + ((size_t)p * 4 + plane0 + m) * wplane;
  for (int g = 0; g < ng; ++g)
    if (lane < N) o[(size_t)g * ld + lane] &= (uint16_t)(sel >> (16 * g));
}

// acoss_binarize_mutual: the made-up bank (n_blocks = {rows0, cols0, rows1, cols1, ...}, pairs (2 b, 2 b + 1)); a matrix
// with no rows or columns, or more than the call's maxima, goes to bad[0].
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

// ---- launchers (ef_internal.hpp) -------------------------------------------------------------------
int ef_launch_rowbin(const float* C, int64_t mstride, int ld, const EfPairs& E, int P, double kappa, uint16_t* Wb,
                     int64_t wplane, int plane0, int nplanes, hipStream_t st) {
  // one binarize block per (pair, matrix) when every track has at most 64 blocks (15,000 Da-TACOS-
  // shape songs: 4.04M -> 4.38M pairs/s, profiles/r05/ef_short/efbin15k_*.log)
  const bool small_bin = ld <= 64;
  // ... and one wave per (pair, matrix) with a row per lane when every row's nn is small (the nn
  // rounds cost nn passes over the row's registers); ACOSS_EF_LANEBIN=0 keeps k_ef_binarize_small
  static const bool lanebin_env = !(getenv("ACOSS_EF_LANEBIN") && getenv("ACOSS_EF_LANEBIN")[0] == '0');
  const bool lane_bin = small_bin && lanebin_env && ef_count(kappa, 64) <= 8;
  if (lane_bin)
    hipLaunchKernelGGL(k_ef_binarize_lanes, dim3((unsigned)((nplanes * P + 3) / 4)), dim3(256), 0, st, C, mstride, ld,
                       E, kappa, Wb, wplane, plane0, nplanes, nplanes * P);
  else if (small_bin)
    hipLaunchKernelGGL(k_ef_binarize_small, dim3(P, nplanes), dim3(256), 0, st, C, mstride, ld, E, kappa, Wb, wplane,
                       plane0);
  else  // k_ef_binarize keeps one u32 per column in LDS
    hipLaunchKernelGGL(k_ef_binarize, dim3((ld + 15) / 16, P, nplanes), dim3(1024), (size_t)ld * 4, st, C, mstride, ld,
                       E, kappa, Wb, wplane, plane0);
  ACOSS_LAUNCH_CHECK();
  return ACOSS_OK;
}

int ef_launch_rowbin_snf(const double* cr, int ld, const EfPairs& E, int P, int K, double kappa, uint16_t* Wb,
                         int64_t wplane, hipStream_t st) {
  hipLaunchKernelGGL(k_efs_binarize, dim3((ld + 15) / 16, P), dim3(256), (size_t)ld * (4 * 8 + 4), st, cr, ld, E, K,
                     kappa, Wb, wplane);
  ACOSS_LAUNCH_CHECK();
  return ACOSS_OK;
}

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
