// ef_csm.hip — the per-track preparation and the three cross-similarity matrices of EarlyFusion
// (acoss/algorithms/earlyfusion_traile.py:173-178), as earlyfusion.hip (the four scores) and
// ef_snf.hip (the per-pair similarity network fusion) share them through ef_internal.hpp.
//
// Per pair (a, b) with beat-synchronous block features (M = n_blocks[a] rows, N = n_blocks[b]):
//   CSM_m = get_csm(mfccs_a, mfccs_b)              euclid, d = 1000   (:173)
//   CSM_s = get_csm(ssms_a, ssms_b)                euclid, d = 1225   (:175)
//   CSM_c = get_csm_blocked_oti(chromas_a, chromas_b, med_a, med_b, get_csm_cosine)  d = 480 (:178)
// ef_prepare, once per call:
//   k_ef_rows      per block row: squared norm (euclid) / L2-normalised copy (cosine; zero -> 1)
//   k_ef_pad_rows  the SSM bank with rows padded to a multiple of 4 floats (the wave-tile kernels'
//                  16-byte loads)
// ef_launch_csms, once per chunk of P pairs (every matrix at pitch ld):
//   k_ef_oti       per pair: get_oti(med_a, med_b), first maximum
//   the wave-tile kernels (rows of d % 4 == 0 floats, chroma rows of d % 24 == 0): one wave per
//   tile of 32x32x2 f32 MFMAs, operands straight from registers, all three on ef_wave_dot:
//     k_ef_csm_w<KIND, TILE>  a 64 x 64 (2 x 2 accumulators) or 32 x 32 tile of one pair
//     k_ef_csm_w4<1, PP>      short tracks, cosine: PP consecutive pairs sharing their query rows
//     k_ef_csm_pack<NB>       short tracks, euclid: the reference columns of a query's run packed
//   k_ef_csm<KIND> any other width (and every width with ACOSS_EF_LDS_CSM set): 64 x 64 tiles of a
//                  256-thread block through two LDS buffers
// Every kernel gives each output the same ascending-k fmaf chain and the same epilogue
// (ef_csm_value), so the CSMs do not depend on the kernel chosen: bit-identical, and equal to the
// canonical CPU oracle (oracle/ef_oracle.cpp). Against the reference only the GEMMs' summation
// order differs (BLAS there, MFMA here).
#include <cstdlib>

#include "common.hpp"
#include "ef_internal.hpp"

namespace acoss {

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
constexpr int kT = 64, kKC = 32;

__global__ void k_ef_rows(const float* __restrict__ X, int64_t nrows, int d, int normalise, float* __restrict__ Xo,
                          float* __restrict__ sq) {
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= nrows) return;
  const float* x = X + row * d;
  float s = 0.0f;
  for (int c = lane; c < d; c += 64) s += x[c] * x[c];
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if (!normalise) {
    if (lane == 0) sq[row] = s;
    return;
  }
  const float nrm = sqrtf(s);
  const float den = nrm != 0.0f ? nrm : 1.0f;  // XNorm[XNorm == 0] = 1 (cross_recurrence.py:67-70)
  for (int c = lane; c < d; c += 64) Xo[row * d + c] = x[c] / den;
}

__global__ void k_ef_oti(const float* __restrict__ med, const int32_t* __restrict__ pairs, int P,
                         int* __restrict__ oti) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= P) return;
  const float* a = med + pairs[2 * p] * 12;
  const float* b = med + pairs[2 * p + 1] * 12;
  int best = 0;
  float bv = 0.0f;
  for (int i = 0; i < 12; ++i) {
    float s = 0.0f;
    for (int c = 0; c < 12; ++c) s = s + a[(c - i + 12) % 12] * b[c];
    if (i == 0 || s > bv) {
      bv = s;
      best = i;
    }
  }
  oti[p] = best;
}

// A CSM entry from its dot product: 1 - dot of the pre-normalised rows (KIND 1, cosine; the squared
// norms are not read) or sqrt(max(0, (|x|^2 + |y|^2) - 2 dot)) (KIND 0, euclid).
template <int KIND>
__device__ __forceinline__ float ef_csm_value(float acc, float sq_row, float sq_col) {
  if constexpr (KIND == 1) return 1.0f - acc;
  float c2 = (sq_row + sq_col) - 2.0f * acc;
  if (c2 < 0.0f) c2 = 0.0f;
  return sqrtf(c2);
}

template <int KIND>  // 0 euclid, 1 cosine (pre-normalised rows, query blocks rolled by oti)
__global__ __launch_bounds__(256) void k_ef_csm(const float* __restrict__ bank, int d, const float* __restrict__ sq,
                                                EfPairs E, const int* __restrict__ oti, int ld,
                                                float* __restrict__ out) {
  // two LDS buffers: the next K chunk is loaded into registers while the MFMAs read this one,
  // then stored to the other buffer; one barrier per chunk
  __shared__ float Xs[2][kT][kKC + 1];
  __shared__ float Ys[2][kT][kKC + 1];
  // 1-D grid of tiles x tiles x pairs, XCD-aware: the tiles of one pair run on one XCD, so its
  // row and column panels are read into that XCD's L2 once and reused by the pair's other tiles
  const int tiles = (ld + kT - 1) / kT;
  const int lg = xcd_remap((int)blockIdx.x, (int)gridDim.x);
  const int p = lg / (tiles * tiles), tix = lg - p * tiles * tiles;
  int a, b, M, N;
  pair_dims(E, p, &a, &b, &M, &N);
  const int bi = (tix / tiles) * kT, bj = (tix % tiles) * kT;
  if (bi >= M || bj >= N) return;
  const float* X = bank + E.off[a] * d;
  const float* Y = bank + E.off[b] * d;
  const int roll = KIND == 1 ? oti[p] : 0;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int wr = w >> 1, wc = w & 1;
  // loader: per load i, lane t reads row t / 32 + 8 i, k = k0 + t % 32 (32 lanes = one 128-B run)
  constexpr int kPer = kT * kKC / 256;
  const int lc = t % kKC, lr0 = t / kKC;
  float xr[kPer], yr[kPer];
  auto gload = [&](int k0) {
    const int k = k0 + lc;
    int kx = k;
    if (KIND == 1 && roll) {  // X1 = np.roll(X blocks, oti, axis=2): X1[k] = X[blk*12 + (cc - oti) mod 12]
      const int blk = k / 12, cc = k - blk * 12;
      kx = blk * 12 + (cc - roll + 12) % 12;
    }
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
      const int r = lr0 + (256 / kKC) * i;
      xr[i] = (bi + r < M && k < d) ? X[(size_t)(bi + r) * d + kx] : 0.0f;
      yr[i] = (bj + r < N && k < d) ? Y[(size_t)(bj + r) * d + k] : 0.0f;
    }
  };
  auto sstore = [&](int buf) {
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
      Xs[buf][lr0 + (256 / kKC) * i][lc] = xr[i];
      Ys[buf][lr0 + (256 / kKC) * i][lc] = yr[i];
    }
  };
  f32x16 acc = {};
  gload(0);
  sstore(0);
  __syncthreads();
  int buf = 0;
  for (int k0 = 0; k0 < d; k0 += kKC) {
    const bool more = k0 + kKC < d;
    if (more) gload(k0 + kKC);
#pragma unroll
    for (int kk = 0; kk < kKC; kk += 2) {
      const float xa = Xs[buf][32 * wr + (lane & 31)][kk + (lane >> 5)];
      const float yb = Ys[buf][32 * wc + (lane & 31)][kk + (lane >> 5)];
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(xa, yb, acc, 0, 0, 0);
    }
    if (more) sstore(buf ^ 1);
    __syncthreads();
    buf ^= 1;
  }
  float* o = out + (size_t)p * ld * ld;
  const int col = bj + 32 * wc + (lane & 31);
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) {
    const int row = bi + 32 * wr + (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5);
    if (row < M && col < N)
      o[(size_t)row * ld + col] = ef_csm_value<KIND>(acc[reg], KIND == 1 ? 0.0f : sq[E.off[a] + row],
                                                     KIND == 1 ? 0.0f : sq[E.off[b] + col]);
  }
}

// Row-padded copy of a feature bank (nrows x d -> nrows x ldp, zeros in [d, ldp)) so that
// the wave-tile kernels' 16-byte row loads are aligned for any d (the SSM blocks have d = 1225).
// The zero columns add exact +0 terms at the end of every fmaf chain, so the CSM is unchanged bit
// for bit.
__global__ void k_ef_pad_rows(const float* __restrict__ X, int64_t nrows, int d, int ldp, float* __restrict__ Xp) {
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= nrows) return;
  for (int c = threadIdx.x & 63; c < ldp; c += 64) Xp[row * ldp + c] = c < d ? X[row * d + c] : 0.0f;
}

// The wave-tile engine: CSM tiles with no LDS and no barriers, one WAVE per tile of 32 x 32
// accumulators of 32x32x2 f32 MFMAs, operands loaded straight into registers. Per block of KB
// k-values, lane l (r = l % 32, h = l / 32) reads KB / 2 contiguous floats of each of its NO
// operand rows (k0 + h KB / 2 ..., 16-byte loads: the two halves cover KB floats of the row),
// and one v_permlane32_swap per register pair turns that into the MFMA layout (step s: half h
// holds k0 + 2 s + h), so every output is the same ascending-k fmaf chain as k_ef_csm:
// bit-identical. Needs d % 4 == 0 (16-byte aligned rows; ef_prepare pads the SSM bank).
#ifndef ACOSS_EF_KB
#define ACOSS_EF_KB 16
#endif
#ifndef ACOSS_EF_DEPTH
#define ACOSS_EF_DEPTH 3
#endif
#ifndef ACOSS_EF_WPE
#define ACOSS_EF_WPE 2
#endif

// The dot products of a lane's NO operand rows over k = 0 .. d - 1. rows[o]: the row's first
// float of this lane's half (row + h KB / 2). mul(block) is called once per whole block of KB
// k-values, in ascending k, with block[o][q] = floats 4 q .. 4 q + 3 of row o's half, and once more
// for the partial tail block (zeros past d). The loads run DEPTH - 1 blocks ahead of the multiplies
// (a ring of register blocks; the last blocks' look-ahead loads are clamped to a valid block and
// never used).
template <int KB, int NO, class Mul>
__device__ __forceinline__ void ef_wave_dot(const float* const (&rows)[NO], int d, int h, const Mul& mul) {
  constexpr int DEPTH = ACOSS_EF_DEPTH, NQ = KB / 8;  // NQ 16-byte loads per row
  const int nfull = d / KB;
  f32x4e ring[DEPTH][NO][NQ];
  auto load = [&](f32x4e (&v)[NO][NQ], int blk) {  // a whole block (clamped to the last whole one)
    const int k0 = min(blk, nfull - 1) * KB;
#pragma unroll
    for (int o = 0; o < NO; ++o)
#pragma unroll
      for (int q = 0; q < NQ; ++q) v[o][q] = *reinterpret_cast<const f32x4e*>(rows[o] + k0 + 4 * q);
  };
  if (nfull > 0) {
#pragma unroll
    for (int i = 0; i < DEPTH - 1; ++i) load(ring[i], i);
#pragma unroll 1
    for (int kb = 0; kb < nfull; kb += DEPTH) {
#pragma unroll
      for (int j = 0; j < DEPTH; ++j) {
        load(ring[(j + DEPTH - 1) % DEPTH], kb + j + DEPTH - 1);
        __builtin_amdgcn_sched_barrier(0);  // keep the loads ahead of the multiplies they overlap
        if (kb + j < nfull) mul(ring[j]);
      }
    }
  }
  if (d % KB) {  // the partial tail block: zeros past d
    const int k0 = nfull * KB;
#pragma unroll
    for (int o = 0; o < NO; ++o)
#pragma unroll
      for (int q = 0; q < NQ; ++q)
        ring[0][o][q] = k0 + (KB / 2) * h + 4 * q < d ? *reinterpret_cast<const f32x4e*>(rows[o] + k0 + 4 * q)
                                                       : f32x4e{0.0f, 0.0f, 0.0f, 0.0f};
    mul(ring[0]);
  }
}

// A block of ef_wave_dot in the MFMA operand layout: operands of steps s and s + KB / 4 come from
// registers 2 s and 2 s + 1 of every operand row.
template <int KB, int NO>
__device__ __forceinline__ void ef_mfma_operands(const f32x4e (&v)[NO][KB / 8], float (&op)[NO][KB / 2]) {
#pragma unroll
  for (int o = 0; o < NO; ++o)
#pragma unroll
    for (int s2 = 0; s2 < KB / 4; ++s2) {
      const float lo = v[o][s2 >> 1][(s2 & 1) * 2], hi = v[o][s2 >> 1][(s2 & 1) * 2 + 1];
      const auto sw = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(unsigned, lo),
                                                       __builtin_bit_cast(unsigned, hi), false, false);
      op[o][s2] = __builtin_bit_cast(float, (unsigned)sw[0]);
      op[o][s2 + KB / 4] = __builtin_bit_cast(float, (unsigned)sw[1]);
    }
}

// The cosine CSM's blocks hold KB = 24 k-values, so each half-wave has one whole 12-bin chroma
// block of a row and the query rows' OTI roll (X1[12 g + c] = X[12 g + (c - oti) mod 12],
// wave-uniform per pair) is a register rotation, spelled out in the multiply steps of k_ef_csm_w<1, .>
// and ef_csm_w4_tiles<1, .>: behind a function of its own, by value or by reference, the same
// rotation changed the register allocation of the cosine kernels (profiles/ef_csm/README.md).

// One tile of one pair per wave. KIND = 1: the cosine chroma CSM of get_csm_blocked_oti
// (pre-normalised rows, 1 - dot); needs d % 24 == 0.
// TILE = 64: 2 x 2 accumulators per wave; TILE = 32: one (the beat-block CSMs of short tracks,
// M, N ~ 14..47 at Da-TACOS lengths, where a 64 x 64 tile is mostly padding).
template <int KIND, int TILE = 64>
__global__ __launch_bounds__(256, ACOSS_EF_WPE) void k_ef_csm_w(const float* __restrict__ bank, int d,
                                                                const float* __restrict__ sq, EfPairs E,
                                                                const int* __restrict__ oti, int ld,
                                                                int n_tiles, float* __restrict__ out) {
  constexpr int KB = KIND == 1 ? 24 : ACOSS_EF_KB, NQ = KB / 8;
  constexpr int NA = TILE / 32;  // 32 x 32 accumulators per tile side
  constexpr int NO = 2 * NA;     // operand rows per lane: NA query rows, then NA reference rows
  const int tiles = (ld + TILE - 1) / TILE;
  const int lb = xcd_remap((int)blockIdx.x, (int)gridDim.x);
  const int tile = lb * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (tile >= n_tiles) return;
  const int p = tile / (tiles * tiles), tix = tile - p * tiles * tiles;
  int a, b, M, N;
  pair_dims(E, p, &a, &b, &M, &N);
  const int bi = (tix / tiles) * TILE, bj = (tix % tiles) * TILE;
  if (bi >= M || bj >= N) return;
  const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
  // this lane's operand rows (clamped into the track: rows past M / N are never stored)
  const float* rows[NO];
#pragma unroll
  for (int o = 0; o < NA; ++o) {
    rows[o] = bank + (E.off[a] + min(bi + 32 * o + r, M - 1)) * (int64_t)d + (KB / 2) * h;
    rows[NA + o] = bank + (E.off[b] + min(bj + 32 * o + r, N - 1)) * (int64_t)d + (KB / 2) * h;
  }
  f32x16 acc[NA][NA] = {};
  const int roll = KIND == 1 ? __builtin_amdgcn_readfirstlane(oti[p]) : 0;
  ef_wave_dot<KB, NO>(rows, d, h, [&](const f32x4e (&vin)[NO][NQ]) {
    f32x4e v[NO][NQ];
#pragma unroll
    for (int o = 0; o < NO; ++o)
#pragma unroll
      for (int q = 0; q < NQ; ++q) v[o][q] = vin[o][q];
    if constexpr (KIND == 1) {  // rotate the query rows' 12-bin block by the pair's OTI
      if (roll) {
#pragma unroll
        for (int o = 0; o < NA; ++o) {
          float e[12], t[12];
#pragma unroll
          for (int c = 0; c < 12; ++c) e[c] = vin[o][c >> 2][c & 3];
#pragma unroll
          for (int R = 1; R < 12; ++R)
            if (roll == R) {
#pragma unroll
              for (int c = 0; c < 12; ++c) t[c] = e[(c - R + 12) % 12];
            }
#pragma unroll
          for (int c = 0; c < 12; ++c) v[o][c >> 2][c & 3] = t[c];
        }
      }
    }
    float op[NO][KB / 2];
    ef_mfma_operands<KB, NO>(v, op);
#pragma unroll
    for (int st = 0; st < KB / 2; ++st)
#pragma unroll
      for (int ti = 0; ti < NA; ++ti)
#pragma unroll
        for (int tj = 0; tj < NA; ++tj)
          acc[ti][tj] = __builtin_amdgcn_mfma_f32_32x32x2f32(op[ti][st], op[NA + tj][st], acc[ti][tj], 0, 0, 0);
  });
  float* ob = out + (size_t)p * ld * ld;
#pragma unroll
  for (int ti = 0; ti < NA; ++ti)
#pragma unroll
    for (int tj = 0; tj < NA; ++tj) {
      const int col = bj + 32 * tj + r;
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) {
        const int row = bi + 32 * ti + (reg & 3) + 8 * (reg >> 2) + 4 * h;
        if (row < M && col < N)
          ob[(size_t)row * ld + col] = ef_csm_value<KIND>(acc[ti][tj][reg], KIND == 1 ? 0.0f : sq[E.off[a] + row],
                                                          KIND == 1 ? 0.0f : sq[E.off[b] + col]);
      }
    }
}

// Short tracks (every track <= 64 blocks: the 32 x 32 tiles of k_ef_csm_w<KIND, 32>), PP pairs per
// wave. The pairs of a call come in (reference band, query) order, so runs of consecutive pairs
// share their query track: a wave takes PP consecutive pairs and, when they share it, loads the
// query rows once for all PP tiles (1 + PP row loads per block instead of 2 PP) and keeps PP
// independent accumulators in flight. Otherwise (a run boundary) it takes the pairs one at a time.
// Each output is the same ascending-k fmaf chain as k_ef_csm_w: bit-identical. Used for the cosine
// chroma CSM (-12 %); the euclid CSMs did not gain (profiles/r06/ef_short_w4/README.txt). Work unit:
// (group of PP pairs, tile row ti, tile column tj).
// pairs per wave of the cosine chroma CSM of short tracks. The euclid CSMs (d = 1000, 1228) keep one
// pair per wave: 2 or 4 pairs sharing the query rows, and a deeper load ring, left them within
// +-5 % (profiles/r06/ef_short_w4/README.txt); the cosine one (d = 480, 24-k blocks) is 12 % faster
// with 2 (4: 40 % slower, registers)
constexpr int kEfPPc = 2;

template <int KIND, int PP>
__device__ __forceinline__ void ef_csm_w4_tiles(const float* __restrict__ bank, int d, const float* __restrict__ sq,
                                                const EfPairs& E, const int* __restrict__ oti, int ld, int pbase,
                                                int npp, int ti, int tj, float* __restrict__ out) {
  constexpr int KB = KIND == 1 ? 24 : ACOSS_EF_KB, NQ = KB / 8;
  constexpr int NO = 1 + PP;  // operand rows per lane: the query row, then one reference row per pair
  const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
  const int a = E.pairs[2 * pbase], M = E.nb[a];
  const int bi = ti * 32, bj = tj * 32;
  int bq[PP], Nq[PP];
  const float* rows[NO];
  rows[0] = bank + (E.off[a] + min(bi + r, M - 1)) * (int64_t)d + (KB / 2) * h;
#pragma unroll
  for (int q = 0; q < PP; ++q) {
    const int qq = min(q, npp - 1);  // pairs past the group's end repeat its last one (never stored)
    bq[q] = E.pairs[2 * (pbase + qq) + 1];
    Nq[q] = E.nb[bq[q]];
    rows[1 + q] = bank + (E.off[bq[q]] + min(bj + r, Nq[q] - 1)) * (int64_t)d + (KB / 2) * h;
  }
  f32x16 acc[PP] = {};
  int roll[PP];
#pragma unroll
  for (int q = 0; q < PP; ++q) roll[q] = KIND == 1 ? __builtin_amdgcn_readfirstlane(oti[pbase + min(q, npp - 1)]) : 0;
  ef_wave_dot<KB, NO>(rows, d, h, [&](const f32x4e (&vin)[NO][NQ]) {
    float op[NO][KB / 2];
    ef_mfma_operands<KB, NO>(vin, op);
#pragma unroll
    for (int q = 0; q < PP; ++q) {
      float oq[1][KB / 2];  // the query operand, rolled by pair q's OTI (cosine)
#pragma unroll
      for (int st = 0; st < KB / 2; ++st) oq[0][st] = op[0][st];
      if constexpr (KIND == 1) {
        if (roll[q]) {  // the query row's 12-bin block rotated, as k_ef_csm_w<1> does before the swap
          float e[12], t[12];
#pragma unroll
          for (int c = 0; c < 12; ++c) e[c] = vin[0][c >> 2][c & 3];
#pragma unroll
          for (int R = 1; R < 12; ++R)
            if (roll[q] == R) {
#pragma unroll
              for (int c = 0; c < 12; ++c) t[c] = e[(c - R + 12) % 12];
            }
          f32x4e vq[1][NQ];
#pragma unroll
          for (int c = 0; c < 12; ++c) vq[0][c >> 2][c & 3] = t[c];
          ef_mfma_operands<KB, 1>(vq, oq);
        }
      }
#pragma unroll
      for (int st = 0; st < KB / 2; ++st)
        acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(oq[0][st], op[1 + q][st], acc[q], 0, 0, 0);
    }
  });
#pragma unroll
  for (int q = 0; q < PP; ++q) {
    if (q >= npp) break;
    float* ob = out + (size_t)(pbase + q) * ld * ld;
    const int col = bj + r;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      const int row = bi + (reg & 3) + 8 * (reg >> 2) + 4 * h;
      if (row < M && col < Nq[q])
        ob[(size_t)row * ld + col] = ef_csm_value<KIND>(acc[q][reg], KIND == 1 ? 0.0f : sq[E.off[a] + row],
                                                        KIND == 1 ? 0.0f : sq[E.off[bq[q]] + col]);
    }
  }
}

template <int KIND, int PP>
__global__ __launch_bounds__(256, ACOSS_EF_WPE) void k_ef_csm_w4(const float* __restrict__ bank, int d,
                                                                 const float* __restrict__ sq, EfPairs E,
                                                                 const int* __restrict__ oti, int ld, int n_pairs,
                                                                 int n_units, float* __restrict__ out) {
  const int tiles = (ld + 31) / 32;
  const int lb = xcd_remap((int)blockIdx.x, (int)gridDim.x);
  const int unit = lb * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (unit >= n_units) return;
  const int g = unit / (tiles * tiles), tix = unit - g * tiles * tiles;
  const int ti = tix / tiles, tj = tix - ti * tiles;
  const int p0 = g * PP, npp = min(PP, n_pairs - p0);
  bool same = true;  // wave-uniform: every pair of the group has the group's query track
  for (int q = 1; q < npp; ++q) same = same && E.pairs[2 * (p0 + q)] == E.pairs[2 * p0];
  // a pair's tile (ti, tj) exists when both tracks reach it; ragged tracks (14..47 blocks at
  // Da-TACOS lengths) leave many groups where only some pairs reach tile column tj
  int nv = 0;
  for (int q = 0; q < npp; ++q)
    nv += (ti * 32 < E.nb[E.pairs[2 * (p0 + q)]] && tj * 32 < E.nb[E.pairs[2 * (p0 + q) + 1]]) ? 1 : 0;
  if (same && nv == npp) {
    ef_csm_w4_tiles<KIND, PP>(bank, d, sq, E, oti, ld, p0, npp, ti, tj, out);
    return;
  }
  for (int q = 0; q < npp; ++q)  // a run boundary or a partial group: one pair at a time
    if (ti * 32 < E.nb[E.pairs[2 * (p0 + q)]] && tj * 32 < E.nb[E.pairs[2 * (p0 + q) + 1]])
      ef_csm_w4_tiles<KIND, 1>(bank, d, sq, E, oti, ld, p0 + q, 1, ti, tj, out);
}

// Euclidean CSMs of short tracks (<= 128 blocks) with the reference columns PACKED: the pairs of a
// call come in (reference band, query) order, so consecutive pairs share their query track; the
// columns of a run of such pairs (all blocks of every reference track, concatenated) fill
// 32 NB-wide tiles with no per-pair padding. A tile per pair wastes the part of the tile past the
// track's block count (14..47 blocks at Da-TACOS lengths: 2.3x the useful MFMA work over rows and
// columns with 32 x 32 tiles); packing leaves only the rows' padding (1.5x). Lane r of a tile
// holds NB packed columns, each with its own reference track, block and output pair, so the same
// 32x32x2 MFMA chains as k_ef_csm_w<0, .> compute every output (bit-identical: the same operands in
// the same ascending-k fmaf order). Work unit: (group of kEfPack consecutive pairs, row tile ti,
// packed column tile tc). Within a group the maximal runs of one query track are packed
// separately; tc counts the runs' tiles in order (at most kEfPack * ceil(ld / 32 NB) of them, so
// that is the grid's column-tile count).
template <int NB>  // packed columns per wave tile: 32 * NB (NB accumulators sharing the query rows)
__global__ __launch_bounds__(256, 4) void k_ef_csm_pack(const float* __restrict__ bank, int d,
                                                                   const float* __restrict__ sq, EfPairs E, int ld,
                                                                   int n_pairs, int n_units, float* __restrict__ out) {
  constexpr int KB = ACOSS_EF_KB, NQ = KB / 8, TW = 32 * NB, NO = 1 + NB;
  const int wt = (ld + 31) / 32;                // row tiles per track
  const int ct = kEfPack * ((ld + TW - 1) / TW);  // column-tile slots per group
  const int lb = xcd_remap((int)blockIdx.x, (int)gridDim.x);
  const int unit = lb * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (unit >= n_units) return;
  const int g = unit / (wt * ct), u = unit - g * wt * ct;
  const int p0 = g * kEfPack, npp = min(kEfPack, n_pairs - p0);
  const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
  // the group's pairs, one per lane (lanes < npp), in two rounds of loads; the walk below reads
  // them with readlane (a chain of dependent scalar loads here cost more than the tile's MFMAs)
  int ga = 0, gb = 0;
  if (lane < npp) {
    ga = E.pairs[2 * (p0 + lane)];
    gb = E.pairs[2 * (p0 + lane) + 1];
  }
  int gm = 0, gn = 0;
  int64_t goa = 0, gob = 0;
  if (lane < npp) {
    gm = E.nb[ga];
    gn = E.nb[gb];
    goa = E.off[ga];
    gob = E.off[gb];
  }
  auto rl64 = [](int64_t v, int l) {
    return ((int64_t)__builtin_amdgcn_readlane((int)(v >> 32), l) << 32) |
           (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, l);
  };
  // Walk the group's SUPER-RUNS: a run of L pairs with one query track, extended by the following
  // runs of L pairs whose reference tracks are the same, in the same order (the next queries of a
  // reference band). A super-run of R queries packs its R queries' blocks into the rows and its L
  // references' blocks into the columns: (query k, reference t) is pair s + k L + t. Its tiles
  // are ceil(sum M / 32) x ceil(sum N / TW); u counts the super-runs' tiles in order (at most the
  // per-pair tile count, so the grid's wt * ct slots per group hold them).
  int s0 = 0, L = 0, R = 0, sumM = 0, sumN = 0, tb = 0, nct = 1;
  bool found = false;
  while (s0 < npp) {
    const int a = __builtin_amdgcn_readlane(ga, s0);
    int e = s0 + 1;
    while (e < npp && __builtin_amdgcn_readlane(ga, e) == a) ++e;
    L = e - s0;
    sumN = 0;
    for (int t = s0; t < e; ++t) sumN += __builtin_amdgcn_readlane(gn, t);
    sumM = __builtin_amdgcn_readlane(gm, s0);
    R = 1;
    int f = e;
    while (f + L <= npp) {  // absorb the next run if it is L pairs with the same references
      const int a2 = __builtin_amdgcn_readlane(ga, f);
      bool same = f + L == npp || __builtin_amdgcn_readlane(ga, f + L) != a2;
      for (int t = 0; t < L && same; ++t)
        same = __builtin_amdgcn_readlane(ga, f + t) == a2 &&
               __builtin_amdgcn_readlane(gb, f + t) == __builtin_amdgcn_readlane(gb, s0 + t);
      if (!same) break;
      sumM += __builtin_amdgcn_readlane(gm, f);
      ++R;
      f += L;
    }
    nct = (sumN + TW - 1) / TW;
    const int nt = (sumM + 31) / 32 * nct;
    if (u < tb + nt) {
      found = true;
      break;
    }
    tb += nt;
    s0 = f;
  }
  if (!found) return;
  const int rt = (u - tb) / nct, tc = (u - tb) - rt * nct;
  // packed row gr -> (query k of the super-run, block within it); rows past sum M clamp to the last.
  // Every lane runs every iteration and selects (no per-lane exit from a loop over readlane
  // values: a value a lane keeps from an earlier iteration than its neighbours is divergent,
  // which the compiler must not mistake for the uniform loop counter)
  auto locate_row = [&](int gr, int* k, int* row, int64_t* offa) {
    int pre = 0, kk_ = R - 1, row_ = 0;
    int64_t off_ = 0;
    bool done = false;
    for (int kk = 0; kk < R; ++kk) {
      const int m = __builtin_amdgcn_readlane(gm, s0 + kk * L);
      const int64_t o = rl64(goa, s0 + kk * L);
      const bool hit = !done && (gr < pre + m || kk == R - 1);
      kk_ = hit ? kk : kk_;
      row_ = hit ? min(gr - pre, m - 1) : row_;
      off_ = hit ? o : off_;
      done = done || hit;
      pre += m;
    }
    *k = kk_;
    *row = row_;
    *offa = off_;
  };
  const float* rows[NO];
  {
    int k, row;
    int64_t offa;
    locate_row(rt * 32 + r, &k, &row, &offa);
    rows[0] = bank + (offa + row) * (int64_t)d + (KB / 2) * h;
  }
  // this lane's packed columns (one per accumulator): reference t of the super-run, block c
  int ct_[NB], cc[NB];
  int64_t cob[NB];
  bool cvalid[NB];
#pragma unroll
  for (int j = 0; j < NB; ++j) {
    const int gc = tc * TW + 32 * j + r;
    cvalid[j] = gc < sumN;
    int t = L - 1, pre = 0, cpre = 0, N = 1;
    int64_t offb = 0;
    bool done = false;
    for (int k = 0; k < L; ++k) {  // the last reference takes every column past the others
      const int n = __builtin_amdgcn_readlane(gn, s0 + k);
      const int64_t o = rl64(gob, s0 + k);
      const bool hit = !done && (gc < pre + n || k == L - 1);
      t = hit ? k : t;
      N = hit ? n : N;
      cpre = hit ? pre : cpre;
      offb = hit ? o : offb;
      done = done || hit;
      pre += n;
    }
    ct_[j] = t;
    cc[j] = min(gc - cpre, N - 1);  // clamped for the padding lanes (never stored)
    cob[j] = offb;
    rows[1 + j] = bank + (offb + cc[j]) * (int64_t)d + (KB / 2) * h;
  }
  f32x16 acc[NB] = {};
  ef_wave_dot<KB, NO>(rows, d, h, [&](const f32x4e (&vin)[NO][NQ]) {
    float op[NO][KB / 2];
    ef_mfma_operands<KB, NO>(vin, op);
#pragma unroll
    for (int st = 0; st < KB / 2; ++st)
#pragma unroll
      for (int j = 0; j < NB; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(op[0][st], op[1 + j][st], acc[j], 0, 0, 0);
  });
  float sqc[NB];
#pragma unroll
  for (int j = 0; j < NB; ++j) sqc[j] = sq[cob[j] + cc[j]];
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) {
    const int gr = rt * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * h;
    if (gr >= sumM) continue;
    int k, row;
    int64_t offa;
    locate_row(gr, &k, &row, &offa);
    const float sqr = sq[offa + row];
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      if (!cvalid[j]) continue;
      out[(size_t)(p0 + s0 + k * L + ct_[j]) * ld * ld + (size_t)row * ld + cc[j]] =
          ef_csm_value<0>(acc[j][reg], sqr, sqc[j]);
    }
  }
}

}  // namespace

int ef_prepare(const EfBank& B, hipStream_t s, EfPrep* out) {
  // per-track scratch: squared norms of the MFCC and SSM blocks, normalised chroma blocks; the
  // caller's block_off / n_blocks give the total row count through the last track
  int64_t h_off = 0;
  int32_t h_nb = 0;
  ACOSS_HIP_CHECK(hipMemcpy(&h_off, B.block_off + (B.n_tracks - 1), 8, hipMemcpyDeviceToHost));
  ACOSS_HIP_CHECK(hipMemcpy(&h_nb, B.n_blocks + (B.n_tracks - 1), 4, hipMemcpyDeviceToHost));
  const int64_t nrows = h_off + h_nb;
  const size_t tr_bytes = align_up((size_t)nrows * 4, 256) * 2 + align_up((size_t)nrows * B.d_chroma * 4, 256);
  char* tws = static_cast<char*>(workspace(10, tr_bytes));
  if (!tws) return ACOSS_E_HIP;
  float* sq_m = reinterpret_cast<float*>(tws);
  float* sq_s = reinterpret_cast<float*>(tws + align_up((size_t)nrows * 4, 256));
  float* chn = reinterpret_cast<float*>(tws + 2 * align_up((size_t)nrows * 4, 256));
  prof_begin(PH_CSM, s);
  const unsigned rb = (unsigned)((nrows + 3) / 4);
  hipLaunchKernelGGL(k_ef_rows, dim3(rb), dim3(256), 0, s, B.mfcc, nrows, B.d_mfcc, 0, nullptr, sq_m);
  ACOSS_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_ef_rows, dim3(rb), dim3(256), 0, s, B.ssm, nrows, B.d_ssm, 0, nullptr, sq_s);
  ACOSS_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_ef_rows, dim3(rb), dim3(256), 0, s, B.chroma, nrows, B.d_chroma, 1, chn, nullptr);
  ACOSS_LAUNCH_CHECK();
  static const bool wave_tiles = getenv("ACOSS_EF_LDS_CSM") == nullptr;
  const float* ssm_p = nullptr;  // SSM bank with rows padded to a multiple of 4 (the wave-tile kernels)
  if (wave_tiles && B.d_ssm % 4 != 0) {
    const int ldp = (int)align_up((size_t)B.d_ssm, 4);
    float* pb = static_cast<float*>(workspace(15, (size_t)nrows * ldp * 4));
    if (!pb) return ACOSS_E_HIP;
    hipLaunchKernelGGL(k_ef_pad_rows, dim3(rb), dim3(256), 0, s, B.ssm, nrows, B.d_ssm, ldp, pb);
    ACOSS_LAUNCH_CHECK();
    ssm_p = pb;
  }
  prof_end(PH_CSM, s);
  *out = EfPrep{sq_m, sq_s, chn, ssm_p, nrows, wave_tiles};
  return ACOSS_OK;
}

int ef_launch_csms(const EfBank& B, const EfPrep& R, const int32_t* pairs, int P, int ld, int* oti, bool self_pairs,
                   float* C, int64_t mstride, hipStream_t st) {
  const bool wave_tiles = R.wave_tiles;
  const EfPairs E{pairs, B.block_off, B.n_blocks};
  const int tiles = (ld + kT - 1) / kT;  // LDS kernel tiles
  // wave-tile CSMs: 32 x 32 tiles when every track has at most 64 blocks (Da-TACOS beat blocks:
  // 14..47, a 64 x 64 tile there is mostly padding; profiles/r05/ef_short), 64 x 64 otherwise
  const int wtile = ld <= 64 ? 32 : 64;
  const int wtiles = (ld + wtile - 1) / wtile;
  auto kw_euclid = wtile == 32 ? k_ef_csm_w<0, 32> : k_ef_csm_w<0, 64>;
  auto kw_cosine = wtile == 32 ? k_ef_csm_w<1, 32> : k_ef_csm_w<1, 64>;
  // short tracks: the cosine CSM with several consecutive pairs per wave sharing their query rows
  // (k_ef_csm_w4); ACOSS_EF_W4=0 keeps one pair per wave
  static const bool w4 = !(getenv("ACOSS_EF_W4") && getenv("ACOSS_EF_W4")[0] == '0');
  // ... and the euclid CSMs with the reference columns of a query's run packed (k_ef_csm_pack):
  // 32 x 64 tiles (pack_nb = 2) for every track up to 128 blocks; ACOSS_EF_PACK=1 takes 32 x 32
  // tiles, 0 a tile per pair (Da-TACOS shapes, profiles/r06/ef_pack/README.txt: 14..47 blocks
  // 4.85M -> 5.72M pairs/s, 30..80 blocks 1.12M -> 1.62M; 32 x 32 tiles 5.68M / 1.59M)
  static const char* pack_env = getenv("ACOSS_EF_PACK");
  const int pack_nb = ld > 128 || (pack_env && pack_env[0] == '0') ? 0 : pack_env && pack_env[0] == '1' ? 1 : 2;
  prof_begin(PH_CSM, st);
  if (self_pairs)
    ACOSS_HIP_CHECK(hipMemsetAsync(oti, 0, (size_t)P * 4, st));
  else
    hipLaunchKernelGGL(k_ef_oti, dim3((P + 255) / 256), dim3(256), 0, st, B.chroma_med, pairs, P, oti);
  ACOSS_LAUNCH_CHECK();
  {
    const int n_tiles = tiles * tiles * P, n_wtiles = wtiles * wtiles * P;
    auto euclid = [&](const float* bank, int d, const float* sq, float* dst) -> int {
      if (wave_tiles && d % 4 != 0 && bank == B.ssm && R.ssm_p) {
        bank = R.ssm_p;  // the row-padded copy made by ef_prepare
        d = (int)align_up((size_t)d, 4);
      }
      if (wave_tiles && d % 4 == 0 && pack_nb) {
        const int tw = 32 * pack_nb;
        const int units = (P + kEfPack - 1) / kEfPack * ((ld + 31) / 32) * (kEfPack * ((ld + tw - 1) / tw));
        hipLaunchKernelGGL(pack_nb == 1 ? k_ef_csm_pack<1> : k_ef_csm_pack<2>, dim3((unsigned)((units + 3) / 4)),
                           dim3(256), 0, st, bank, d, sq, E, ld, P, units, dst);
      } else if (wave_tiles && d % 4 == 0)
        hipLaunchKernelGGL(kw_euclid, dim3((unsigned)((n_wtiles + 3) / 4)), dim3(256), 0, st, bank, d, sq, E, oti, ld,
                           n_wtiles, dst);
      else
        hipLaunchKernelGGL(k_ef_csm<0>, dim3((unsigned)n_tiles), dim3(256), 0, st, bank, d, sq, E, oti, ld, dst);
      ACOSS_LAUNCH_CHECK();
      return ACOSS_OK;
    };
    if (euclid(B.mfcc, B.d_mfcc, R.sq_m, C) != ACOSS_OK || euclid(B.ssm, B.d_ssm, R.sq_s, C + mstride) != ACOSS_OK)
      return ACOSS_E_HIP;
  }
  if (wave_tiles && B.d_chroma % 24 == 0 && w4 && wtile == 32) {
    const int units = (P + kEfPPc - 1) / kEfPPc * wtiles * wtiles;
    hipLaunchKernelGGL((k_ef_csm_w4<1, kEfPPc>), dim3((unsigned)((units + 3) / 4)), dim3(256), 0, st, R.chn,
                       B.d_chroma, nullptr, E, oti, ld, P, units, C + 2 * mstride);
  } else if (wave_tiles && B.d_chroma % 24 == 0)
    hipLaunchKernelGGL(kw_cosine, dim3((unsigned)((wtiles * wtiles * P + 3) / 4)), dim3(256), 0, st, R.chn, B.d_chroma,
                       nullptr, E, oti, ld, wtiles * wtiles * P, C + 2 * mstride);
  else
    hipLaunchKernelGGL(k_ef_csm<1>, dim3((unsigned)(tiles * tiles * P)), dim3(256), 0, st, R.chn, B.d_chroma, nullptr, E,
                       oti, ld, C + 2 * mstride);
  ACOSS_LAUNCH_CHECK();
  prof_end(PH_CSM, st);
  return ACOSS_OK;
}

}  // namespace acoss
