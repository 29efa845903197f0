// ef_internal.hpp — the per-track preparation and the three CSMs of EarlyFusion, as earlyfusion.hip
// (the four scores) and ef_snf.hip (the per-pair similarity network fusion) share them.
#pragma once
#include "common.hpp"

namespace acoss {

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

// Per-track scratch of a call: squared norms of the MFCC and SSM blocks, L2-normalised chroma
// blocks and, where d_ssm is no multiple of 4, the row-padded SSM bank (workspace slots 10, 15).
struct EfPrep {
  const float *sq_m, *sq_s, *chn, *ssm_p;
  int64_t nrows;
};
int ef_prepare(const EfBank& B, hipStream_t s, EfPrep* out);

// The three CSMs (mfccs, ssms, chromas) of P pairs into C + f * mstride + p * ld * ld (row pitch
// ld, a multiple of 4). oti: int[P] scratch; with self_pairs it is zeroed (pairs (t, t): the plain
// distances of a track against itself, no roll), otherwise filled with get_oti of each pair.
int ef_launch_csms(const EfBank& B, const EfPrep& R, const int32_t* pairs, int P, int ld, int* oti, bool self_pairs,
                   float* C, int64_t mstride, hipStream_t st);

}  // namespace acoss
