// ef_internal.hpp — what earlyfusion.hip (the four scores) and ef_snf.hip (the per-pair similarity
// network fusion) share: the per-track preparation and the three CSMs of EarlyFusion (ef_csm.hip),
// the entries' common argument check and chunk budget, the binarisation launchers (ef_binarize.hip)
// and the Smith-Waterman metadata launch.
#pragma once
#include <cstdlib>

#include "common.hpp"

namespace acoss {

typedef float f32x4e __attribute__((ext_vector_type(4)));

struct EfPairs {
  const int32_t* pairs;
  const int64_t* off;  // block offsets per track
  const int32_t* nb;   // blocks per track
};

__device__ __forceinline__ void pair_dims(const EfPairs& E, int p, int* a, int* b, int* M, int* N) {
  *a = E.pairs[2 * p];
  *b = E.pairs[2 * p + 1];
  *M = E.nb[*a];
  *N = E.nb[*b];
}

// The block bank of a call (device pointers), as the C-ABI entries take it.
struct EfBank {
  const float *mfcc, *ssm, *chroma, *chroma_med;
  const int64_t* block_off;
  const int32_t* n_blocks;
  int32_t n_tracks, d_mfcc, d_ssm, d_chroma;
};

// The bank and pair arguments every EarlyFusion entry takes; `k_max`: the largest K of the entry
// (max_blocks where getWCSM(K, K) runs on the CSM itself, the lane limit for early SNF, whose pairs
// answer for K one by one); `own_bad`: what the entry checks beyond them. Sets "<entry>: bad
// arguments" and returns ACOSS_E_ARG when anything is off.
inline int ef_check_args(const char* entry, const EfBank& B, int32_t max_blocks, const int32_t* pairs, int64_t n_pairs,
                         double kappa, int32_t K, int32_t k_max, const double* scores_out, bool own_bad) {
  if (B.n_tracks <= 0 || n_pairs < 0 || max_blocks <= 0 || B.d_mfcc <= 0 || B.d_ssm <= 0 || B.d_chroma <= 0 ||
      B.d_chroma % 12 != 0 || K <= 0 || K > k_max || kappa < 0.0 || own_bad ||
      (n_pairs > 0 && (!B.mfcc || !B.ssm || !B.chroma || !B.chroma_med || !B.block_off || !B.n_blocks || !pairs ||
                       !scores_out))) {
    set_error("%s: bad arguments", entry);
    return ACOSS_E_ARG;
  }
  return ACOSS_OK;
}

// Bytes of workspace a chunk of pairs may take: 4 GiB, or ACOSS_EF_BYTES.
inline size_t ef_chunk_budget() {
  if (const char* e = getenv("ACOSS_EF_BYTES")) return strtoull(e, nullptr, 10);
  return (size_t)4 << 30;
}

// Per-track scratch of a call: squared norms of the MFCC and SSM blocks, L2-normalised chroma
// blocks and, where d_ssm is no multiple of 4, the row-padded SSM bank (workspace slots 10, 15).
// wave_tiles: the call uses the wave-tile CSM kernels (ACOSS_EF_LDS_CSM unset), read once here so
// that the padded bank and the kernel choice of ef_launch_csms agree.
struct EfPrep {
  const float *sq_m, *sq_s, *chn, *ssm_p;
  int64_t nrows;
  bool wave_tiles;
};
int ef_prepare(const EfBank& B, hipStream_t s, EfPrep* out);

// Pairs per packing group of k_ef_csm_pack (one per lane in its walk); ef_batches starts its chunks
// at multiples of it. With runs of 32 pairs per query, kernel time per 1M Da-TACOS-shape pairs
// 209 / 148 / 94 / 87 / 85 ms for groups of 4 / 8 / 16 / 32 / 64, against 119 ms for a 32 x 32 tile
// per pair (profiles/r06/ef_pack/README.txt)
#ifndef ACOSS_EF_PACKN
#define ACOSS_EF_PACKN 64
#endif
constexpr int kEfPack = ACOSS_EF_PACKN;
static_assert(kEfPack <= 64, "one pair per lane");

// The three CSMs (mfccs, ssms, chromas) of P pairs into C + f * mstride + p * ld * ld (row pitch
// ld, a multiple of 4). oti: int[P] scratch; with self_pairs it is zeroed (pairs (t, t): the plain
// distances of a track against itself, no roll), otherwise filled with get_oti of each pair.
int ef_launch_csms(const EfBank& B, const EfPrep& R, const int32_t* pairs, int P, int ld, int* oti, bool self_pairs,
                   float* C, int64_t mstride, hipStream_t st);

// k1, k2 of getWCSMSSM and whether the reference can fuse the pair at all (early SNF)
__device__ __forceinline__ bool snf_split(int M, int N, int K, int* k1, int* k2) {
  *k1 = (int)((double)K * (double)M / (double)(M + N));
  *k2 = K - *k1;
  return *k1 >= 1 && *k1 <= M - 2 && *k2 >= 1 && *k2 <= N - 2 && K < M + N;
}

// The binarisation launchers (ef_binarize.hip: the rule and the kernel of every shape class). Bit
// planes: Wb, plane stride wplane, ppp per pair (4; 1 for early SNF). rowbin: csm_to_binary over
// `nplanes` CSM planes of P pairs (C + m * mstride + p * ld * ld) into bit planes plane0 .. plane0 +
// nplanes - 1 of each pair's four. colpass: the column half of the mutual rule (the definition:
// include/acoss_hip.h) clears, in those planes, the rows that are not among the count(kappa, M)
// smallest of their column, ties to the lowest row. _snf: the LARGEST of each row / column of early
// SNF's float64 cross planes (cr + p * ld * ld), one bit plane per pair; a pair that snf_split
// refuses gets / keeps an empty plane. unpack: bit plane 0 of each pair's ppp -> its M x N byte
// matrix, row-major at out + off[p].
int ef_launch_rowbin(const float* C, int64_t mstride, int ld, const EfPairs& E, int P, double kappa, uint16_t* Wb,
                     int64_t wplane, int plane0, int nplanes, hipStream_t st);
int ef_launch_colpass(const float* C, int64_t mstride, int ld, const EfPairs& E, int P, double kappa, uint16_t* Wb,
                      int64_t wplane, int plane0, int nplanes, hipStream_t st);
int ef_launch_rowbin_snf(const double* cr, int ld, const EfPairs& E, int P, int K, double kappa, uint16_t* Wb,
                         int64_t wplane, hipStream_t st);
int ef_launch_colpass_snf(const double* cr, int ld, const EfPairs& E, int P, int K, double kappa, uint16_t* Wb,
                          int64_t wplane, hipStream_t st);
int ef_launch_unpack(const uint16_t* Wb, int64_t wplane, int ppp, int ld, const EfPairs& E, int P, const int64_t* off,
                     uint8_t* out, hipStream_t st);

// Smith-Waterman metadata of P pairs with `repeat` matrices each (matrix p * repeat + s of pair p):
// rows = M, cols = N of the pair (earlyfusion.hip).
int ef_launch_swmeta(const EfPairs& E, int P, int repeat, int32_t* rows, int32_t* cols, hipStream_t st);

}  // namespace acoss
