// sw_internal.hpp — the constrained Smith-Waterman walk over bit planes (sw.hip), as earlyfusion.hip
// and ef_snf.hip (the four matrices of a pair) launch it.
#pragma once
#include "common.hpp"

namespace acoss {

// Scores: matrix mid's words start at W + mid * wstride, row stride ldw words (word
// [g][c] holds rows 16 g .. 16 g + 15 of column c); bnd: sw_bnd_bytes per matrix.
size_t sw_bnd_bytes(int max_rows, int max_cols);
int launch_swb_batch(const uint16_t* W, int64_t wstride, int ldw, const int32_t* rows, const int32_t* cols, int n,
                     int max_rows, int max_cols, void* bnd, double* out, hipStream_t s);

// Where the alignment lies (the definition: include/acoss_hip.h, acoss_sw_locate), over
// the same planes, for matrices of at most kSwCellMax rows and columns. Both DPs keep 8 rows per
// lane at every shape. bnd: swt_bnd_bytes per matrix, read and written only by matrices of more
// than 512 rows. score may be NULL.
constexpr int kSwCellMax = 65535;  // 16 bits per coordinate of a packed cell
size_t swt_bnd_bytes(int max_rows, int max_cols);
// seg[mid] = (r0, c0, r1, c1), (-1, -1, -1, -1) where the score is 0
int launch_swt_locate(const uint16_t* W, int64_t wstride, int ldw, const int32_t* rows, const int32_t* cols, int n,
                      int max_rows, int max_cols, void* bnd, double* score, int32_t* seg, hipStream_t s);
// the direction DP into plane (swt_plane_bytes per matrix) and endkey (4 bytes per matrix), then the
// walk back: len[mid] cells (r, c), first to last, at path + 2 path_cap mid, the rest -1; seg may be NULL
size_t swt_plane_bytes(int max_rows, int max_cols);
int launch_swt_path(const uint16_t* W, int64_t wstride, int ldw, const int32_t* rows, const int32_t* cols, int n,
                    int max_rows, int max_cols, void* bnd, void* plane, uint32_t* endkey, double* score, int path_cap,
                    int32_t* seg, int32_t* len, int32_t* path, hipStream_t s);
// the most cells a path of an M x N matrix can have: its cells lie in [2, min(M, N) - 2] and climb
// in both coordinates
__host__ __device__ inline int sw_path_bound(int M, int N) {
  const int b = (M < N ? M : N) - 3;
  return b > 0 ? b : 0;
}

}  // namespace acoss
