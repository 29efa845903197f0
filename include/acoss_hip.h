/*
 * acoss_hip.h — C-ABI of libacoss_hip.so, the MI355X (gfx950) engine for the acoss
 * all-pairs cross-similarity + alignment hot path.
 *
 * Conventions:
 *  - Every array pointer is a DEVICE pointer owned by the caller (torch tensors), unless
 *    the parameter name ends in `_host`. Scalars are passed by value.
 *  - Row-major, C-contiguous. Chroma features are packed: track t occupies rows
 *    [track_off[t], track_off[t] + track_len[t]) of a (sum_len x 12) float32 block.
 *  - Every call is stream-ordered on `hip_stream` (a hipStream_t; NULL = default stream)
 *    and returns 0 on success or a negative ACOSS_E* code. No C++ exception crosses the
 *    ABI; acoss_last_error() returns a thread-local message for the last failure.
 *  - The only allocation is an internal, grow-only device workspace cache
 *    (acoss_release_workspace() frees it).
 *
 * Each entry point cites the reference interface it replaces (paths relative to the
 * reference repo silvadirceu/acoss-1).
 */
#ifndef ACOSS_HIP_H
#define ACOSS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ACOSS_OK 0
#define ACOSS_E_ARG (-1)      /* invalid argument / unsupported parameter */
#define ACOSS_E_SHAPE (-2)    /* track too short for the frame stacking (n <= m*tau) */
#define ACOSS_E_HIP (-3)      /* HIP runtime error */
#define ACOSS_E_NONBINARY (-4)/* non-binary element in an alignment input (alignment_tools.py:22-23) */

/* Parameters of essentia ChromaCrossSimilarity + CoverSongSimilarity as acoss calls them
 * (acoss/algorithms/rqa_serra09.py:31-32,60-64; latefusion_chen.py:58-71). */
typedef struct acoss_crp_params {
  int32_t m;          /* frameStackSize, default 9 */
  int32_t tau;        /* frameStackStride, default 1 */
  float kappa;        /* binarizePercentile, default 0.095 */
  int32_t oti;        /* 1 = optimal transposition of the reference (default), 0 = none */
  float gamma_open;   /* disOnset, default 0.5 */
  float gamma_ext;    /* disExtension, default 0.5 */
} acoss_crp_params;

/* How the two chroma sequences become a binary matrix. acoss_crp_params keeps its layout; the
 * entries ending in 2 (below, after acoss_crp_rqa) take this wider struct and every other argument
 * of the entry they are the twin of.
 *   ACOSS_BIN_PERCENTILE: essentia ChromaCrossSimilarity(binarizePercentile=kappa, oti), the mutual
 *     row / column percentile CRP of the entries without a 2. oti_rank is ignored.
 *   ACOSS_BIN_OTI: the chroma binary similarity of Serra, Gomez, Herrera and Serra, "Chroma binary
 *     similarity and local alignment applied to cover song identification" (IEEE TASLP 2008), the
 *     mode essentia reaches with otiBinary=True. kappa is not read.
 *
 * The definition of ACOSS_BIN_OTI, for a pair (query X, reference Y), m, tau, oti and
 * oti_rank in 1 .. 12:
 *   g = the pair's global OTI exactly as under the percentile CRP (what oti_out reports); 0 when
 *     oti = 0.
 *   D_k(i, j), k = 0 .. 11: the canonical stacked distance of stacked query frame i and stacked
 *     reference frame j with every reference frame rolled by (g + k) mod 12: the float32 value
 *     acoss_crp_pair writes to dist for that roll, bit for bit. That is the fmaf chain over the 12
 *     chroma bins in bin order, the m window taps added in tap order, then
 *     (N_query - 2 dot) + N_reference clamped at +0, N the per-track stacked squared norms of the
 *     UN-rolled track, then the correctly rounded square root. It equals
 *     oracle.crp_dist(X, Y, (g + k) % 12, m, tau).
 *   closer(i, j) = #{k in 1 .. 11 : D_k(i, j) < D_0(i, j)}, a strict comparison of those float32
 *     values.
 *   C(i, j) = 1 iff closer(i, j) < oti_rank.
 * Consequences:
 *   oti_rank = 1 is "transposition 0 is the best, the first maximum wins", Serra08's rule: among
 *     equal distances the smallest shift wins, as np.argmax does in get_oti.
 *   oti_rank = 12 gives all ones; the masks are nested in oti_rank.
 *   A stacked frame that is all zero, on either side, makes all twelve distances equal: its whole
 *     row or column is 1.
 *   Distinct squared distances may round to the same square root; they then count as equal.
 *   The dims M', N' are those of the percentile CRP: ceil((n - m tau) / tau).
 * The definition is on distances, not on dot products: the distance is what the oracle exposes and
 * the kernels reproduce bit for bit. It is this project's own. Parity with essentia's otiBinary is
 * NOT pinned (as for the percentile CRP): whether essentia stacks the frames before the per-cell
 * OTI, and which index set it accepts (one reading accepts indices 0 and 1; oti_rank = 2 is the
 * nearest equivalent here), are undetermined.
 * Every m <= 64 and every tau run one kernel (crp_otib.hip k_crp_otib); no row or column order
 * statistic, no rolled copy of the reference and no distance plane is made.
 * oti_rank outside 1 .. 12 under ACOSS_BIN_OTI, or an unknown binarize, returns ACOSS_E_ARG. */
#define ACOSS_BIN_PERCENTILE 0
#define ACOSS_BIN_OTI 1
typedef struct acoss_crp_params2 {
  acoss_crp_params base;
  int32_t binarize;   /* ACOSS_BIN_PERCENTILE (what the entries without a 2 run) or ACOSS_BIN_OTI */
  int32_t oti_rank;   /* ACOSS_BIN_OTI: 1 .. 12, Serra08's rule is 1; ignored under ACOSS_BIN_PERCENTILE */
} acoss_crp_params2;

/* Library / build information. */
const char* acoss_version(void);
const char* acoss_last_error(void);
int acoss_release_workspace(void);

/* Optional phase timing (bench.py): HIP events recorded around every kernel launch on the
 * launch stream. enable(1) clears and starts recording, enable(0) stops. read() synchronises
 * the events and fills total_ms[i] / count[i] for phase i < n; returns the phase count.
 * Phase names: acoss_profile_phase_name(i). */
int acoss_profile_enable(int on);
int acoss_profile_read(double* total_ms, int64_t* count, int n);
const char* acoss_profile_phase_name(int i);

/* ---------------------------------------------------------------------------------
 * Serra09 / LateFusionChen hot path for a batch of song pairs (A1/A4/A9/A10/A16).
 * Replaces, per pair (i, j) = (pairs[2p], pairs[2p+1]):
 *   crp = essentia.ChromaCrossSimilarity(frameStackSize=m, frameStackStride=tau,
 *                                        binarizePercentile=kappa, oti=oti)(query, reference)
 *   _, qmax = essentia.CoverSongSimilarity('serra09', 'symmetric')(crp)
 *   _, dmax = essentia.CoverSongSimilarity('chen17',  'symmetric')(crp)
 * at acoss/algorithms/rqa_serra09.py:55-69 and acoss/algorithms/latefusion_chen.py:58-73.
 * query = track pairs[2p], reference = track pairs[2p+1]. qmax_out / dmax_out / oti_out are
 * float[n_pairs] / float[n_pairs] / int32[n_pairs] and each may be NULL (not computed).
 * max_len = max track_len over the tracks referenced (host scalar; sizes the workspace).
 * --------------------------------------------------------------------------------- */
int acoss_crp_align(const float* feats, const int64_t* track_off, const int32_t* track_len, int32_t n_tracks,
                    int32_t max_len, const int32_t* pairs, int64_t n_pairs, const acoss_crp_params* params,
                    float* qmax_out, float* dmax_out, int32_t* oti_out, void* hip_stream);

/* Single-pair CRP with every intermediate exposed (parity / debugging of A1/A4).
 * X: (M x 12), Y: (N x 12) device float32. Outputs (device, each may be NULL):
 *   dist (Mp x Np) float32 stacked Euclidean distances, thr_row (Mp), thr_col (Np) float32
 *   percentile thresholds, crp (Mp x Np) uint8 mutual-neighbour mask, oti (1) int32.
 * Mp = ceil((M - m*tau)/tau), Np likewise (essentia stackChromaFrames).
 * thr_row, thr_col and crp come from the kernels acoss_crp_align runs for this shape, as a batch
 * of one pair; dist from the generic panel kernel. */
int acoss_crp_pair(const float* X, int32_t M, const float* Y, int32_t N, const acoss_crp_params* params,
                   float* dist, float* thr_row, float* thr_col, uint8_t* crp, int32_t* oti, void* hip_stream);

/* essentia CoverSongSimilarity(alignmentType, distanceType='symmetric') on a given binary
 * matrix (A9/A10): crp (M x N) uint8 in {0,1}. align = 0 'serra09' (Qmax), 1 'chen17'
 * (dmax). score_out: float[1]. Replaces the alignment calls at rqa_serra09.py:64,67 and
 * latefusion_chen.py:67-71 when the CRP comes from elsewhere. */
int acoss_align_crp(const uint8_t* crp, int32_t M, int32_t N, int32_t align, float gamma_open, float gamma_ext,
                    float* score_out, void* hip_stream);

/* Where the Qmax alignment lies (no counterpart call in the reference, whose CoverSongSimilarity
 * returns the whole score matrix instead): acoss_crp_align's Qmax of every pair together with
 * the first cell, in row-major order, that holds it (i1, j1) and the cell its path began at
 * (i0, j0), by origin propagation inside the DP (crp_dp.hip k_crp_dp_trace); no M' x N' score matrix
 * is written. A path extends through the predecessors (i-1, j-1), (i-2, j-1), (i-1, j-2) in that
 * order, the first one attaining the maximum wins; a hit whose predecessors are all 0 starts one.
 * serra09; acoss_crp_locate_dmax below is its chen17 twin.
 * seg_out: int32[4 n_pairs] = (i0, j0, i1, j1) in stacked-frame rows (query) and
 * columns (reference); qmax_out, oti_out may be NULL; seg_out must not be. A pair whose Qmax is 0
 * gets (-1, -1, -1, -1). The CRP is the one acoss_crp_align computes (same kernels, same
 * workspace), qmax_out is its qmax_out bit for bit. A stacked length above 65,535 returns
 * ACOSS_E_SHAPE (a cell is packed into 16 + 16 bits). */
int acoss_crp_locate(const float* feats, const int64_t* track_off, const int32_t* track_len, int32_t n_tracks,
                     int32_t max_len, const int32_t* pairs, int64_t n_pairs, const acoss_crp_params* params,
                     float* qmax_out, int32_t* seg_out, int32_t* oti_out, void* hip_stream);
/* the same on a given binary matrix (mirrors acoss_align_crp, non-binary input refused alike):
 * score_out float[1], seg_out int32[4]; M or N above 65,535 returns ACOSS_E_SHAPE. */
int acoss_locate_crp(const uint8_t* crp, int32_t M, int32_t N, float gamma_open, float gamma_ext,
                     float* score_out, int32_t* seg_out, void* hip_stream);

/* The Qmax alignment itself: every cell of the path acoss_crp_locate gives the two ends of, i.e.
 * which query frame goes with which reference frame (the reference leaves this backtrack over
 * CoverSongSimilarity's score matrix to its caller). A direction DP (crp_dp.hip k_crp_dp_dir)
 * writes a 2-bit predecessor code per cell to a per-pair plane in the workspace (about M' N' / 4
 * bytes; the plane of one DP batch stays under 4 GiB or ACOSS_PATH_BYTES, by a smaller DP batch
 * where needed), and k_crp_backtrack walks it from the end cell. The path of a pair is the chain
 * of chosen predecessors (same order and tie rule as acoss_crp_locate) from (i1, j1) back to a
 * cell without one, reported from (i0, j0) to (i1, j1): strictly increasing in i and j, steps
 * (1, 1), (2, 1), (1, 2), at most min(M', N') cells, empty where Qmax is 0. serra09; chen17 has
 * acoss_crp_path_dmax below.
 * path_out: int32[n_pairs][path_cap][2] of (i, j) in stacked-frame rows and columns; the first
 * len_out[p] entries of pair p are its path, the others hold -1. path_cap must be at least the
 * stacked length of max_len (ACOSS_E_ARG otherwise; no pair's path is longer). qmax_out, seg_out,
 * oti_out may be NULL, len_out and path_out must not be; seg_out is acoss_crp_locate's and
 * qmax_out acoss_crp_align's, bit for bit (same CRP kernels, same workspace). A stacked length
 * above 65,535 returns ACOSS_E_SHAPE. */
int acoss_crp_path(const float* feats, const int64_t* track_off, const int32_t* track_len, int32_t n_tracks,
                   int32_t max_len, const int32_t* pairs, int64_t n_pairs, const acoss_crp_params* params,
                   float* qmax_out, int32_t* seg_out, int32_t* oti_out, int32_t path_cap, int32_t* len_out,
                   int32_t* path_out, void* hip_stream);
/* the same on a given binary matrix (mirrors acoss_locate_crp, non-binary input refused alike):
 * score_out float[1], seg_out int32[4] (may be NULL), len_out int32[1], path_out
 * int32[path_cap][2]; path_cap below min(M, N) returns ACOSS_E_ARG, M or N above 65,535
 * ACOSS_E_SHAPE. A matrix with fewer than 3 rows or columns has score 0 and an empty path. */
int acoss_path_crp(const uint8_t* crp, int32_t M, int32_t N, float gamma_open, float gamma_ext, float* score_out,
                   int32_t* seg_out, int32_t path_cap, int32_t* len_out, int32_t* path_out, void* hip_stream);

/* Where the dmax (chen17) alignment lies and which cells it passes: the four entries above for the
 * other aligner, argument for argument, with dmax_out in place of qmax_out. dmax_out is
 * acoss_crp_align's dmax_out (score_out acoss_align_crp's at align = 1) bit for bit, whichever of
 * its score kernels that call runs. Same kernels around the same walk (crp_dp.hip
 * k_crp_dp_trace<1, ., .>, k_crp_dp_dir<1, ., .>, k_crp_backtrack_dmax), same workspace, same
 * conventions (seg_out = (i0, j0, i1, j1), path_out padded with -1) and the same refusals.
 *
 * The definition. C is the binary M x N matrix, D the chen17 score matrix of
 * oracle/crp_oracle.cpp or_align(which = 1), all arithmetic float32; cells with i < 2 or j < 2 hold
 * 0; g(c) = gamma_open if c is set, else gamma_ext. The predecessors of X = (i, j), i, j >= 2, in
 * this fixed order, each with the cell it steps over and its raw value:
 *     a: P = (i-1, j-1), no intermediate,  D[P]
 *     b: P = (i-2, j-1), I = (i-1, j),     D[P] + C[I]
 *     c: P = (i-1, j-2), I = (i, j-1),     D[P] + C[I]
 *   score: on a hit D[X] = max(raw) + 1; on a miss D[X] = max(0, max_k (raw_k - g(C[P_k]))).
 *   chosen predecessor: the FIRST of a, b, c attaining the maximum, taken over the raw values on a
 *     hit and over the penalised values on a miss (a strictly greater value replaces, an equal one
 *     does not). A hit whose maximum is 0 has none (a path starts at X), nor has a cell with
 *     D[X] == 0.
 *   path: the chain from the end cell backwards. At X with chosen predecessor k: if I exists and
 *     C[I] is set, I is on the path (the hit the bonus paid for); if D[P] > 0 the chain goes on at
 *     P; otherwise the path begins at I, the only other way a path starts, and I is then a hit.
 *     A P in row or column 0 or 1 has D = 0 whatever C holds there; an I may lie in row 1 or
 *     column 1, it is a real cell of the matrix and is reported, so i0 or j0 may be 1.
 *   end cell: the first cell in row-major order holding dmax; segment: (first path cell, end
 *     cell), (-1, -1, -1, -1) where dmax is 0.
 *   order and steps: from origin to end; steps (1, 1), (2, 1), (1, 2) and, exactly after an
 *     intermediate cell, (1, 0) and (0, 1): non-decreasing in i and j, not strictly increasing.
 *   length: at most floor(2 (M + N) / 3) - 2 cells for M, N >= 3 (a diagonal step adds one cell
 *     for two of rows plus columns, a b or c step two for three, a start on an intermediate one
 *     more; crp_internal.hpp dmax_path_bound has the proof), so more than min(M, N) is possible.
 *   Origins are defined for gamma >= 0, as for Qmax.
 * path_cap must be at least that bound, taken at M = N = the stacked length of max_len for the
 * batch entry (floor(4 L / 3) - 2) and at the matrix' own M, N for acoss_path_crp_dmax:
 * ACOSS_E_ARG otherwise, the message naming the bound. A stacked length, M or N above 65,535
 * returns ACOSS_E_SHAPE, a non-binary matrix ACOSS_E_NONBINARY; a matrix with fewer than 3 rows
 * or columns has score 0 and an empty path. */
int acoss_crp_locate_dmax(const float* feats, const int64_t* track_off, const int32_t* track_len, int32_t n_tracks,
                          int32_t max_len, const int32_t* pairs, int64_t n_pairs, const acoss_crp_params* params,
                          float* dmax_out, int32_t* seg_out, int32_t* oti_out, void* hip_stream);
int acoss_locate_crp_dmax(const uint8_t* crp, int32_t M, int32_t N, float gamma_open, float gamma_ext,
                          float* score_out, int32_t* seg_out, void* hip_stream);
int acoss_crp_path_dmax(const float* feats, const int64_t* track_off, const int32_t* track_len, int32_t n_tracks,
                        int32_t max_len, const int32_t* pairs, int64_t n_pairs, const acoss_crp_params* params,
                        float* dmax_out, int32_t* seg_out, int32_t* oti_out, int32_t path_cap, int32_t* len_out,
                        int32_t* path_out, void* hip_stream);
int acoss_path_crp_dmax(const uint8_t* crp, int32_t M, int32_t N, float gamma_open, float gamma_ext, float* score_out,
                        int32_t* seg_out, int32_t path_cap, int32_t* len_out, int32_t* path_out, void* hip_stream);

/* Cross-recurrence quantification of every pair's CRP (Serra, Serra and Andrzejak 2009 define Lmax,
 * Smax and Qmax on the cross-recurrence plot; the line measures are the standard CRQA ones, Marwan
 * et al. 2007). No counterpart call in the reference, which keeps only Qmax. The CRP is the one
 * acoss_crp_align computes (same kernels, same workspace); the line measures come from one more
 * walk over its words (crp_dp.hip k_crp_rqa).
 *
 * The definition. C is the pair's binary M x N matrix; all M rows and N columns count (the "rows
 * and columns 0 and 1 hold 0" convention belongs to the Q / S score matrices only).
 *   lines: a diagonal line is a maximal run of set cells (i, j), (i+1, j+1), ..., bounded on each
 *     side by an unset cell or the matrix edge. H[l] = the number of lines of length l,
 *     1 <= l <= min(M, N). lmin >= 1 is the shortest line the "min" measures take (2 is the usual
 *     CRQA setting).
 *   integers: n_rec = set cells (= sum l H[l]); n_lines = sum H[l]; n_lines_min = sum_{l >= lmin}
 *     H[l]; n_pts_min = sum_{l >= lmin} l H[l] (int64); lmax = the largest l with H[l] > 0 (int32, 0
 *     for a matrix without a set cell).
 *   float64, each of the first three ONE IEEE division of two exactly representable integers:
 *     RR = n_rec / (M N); DET = n_pts_min / n_rec (0 when n_rec = 0); LMEAN = n_pts_min /
 *     n_lines_min (0 without such lines); ENTR = - sum_{l >= lmin, H[l] > 0} p(l) ln p(l) with
 *     p(l) = H[l] / n_lines_min (0 when n_lines_min = 0), float64 log, a fixed summation order.
 *   Smax: the Q recurrence without its penalties: cells with i < 2 or j < 2 hold 0; on a hit
 *     S = max(S[i-1, j-1], S[i-2, j-1], S[i-1, j-2]) + 1, on a miss S = 0; Smax = max S, float32.
 *     It is acoss_crp_align's Qmax DP at gamma_open = gamma_ext = +inf, and computed by it.
 * counts_out: int64[n_pairs][4] = n_rec, n_lines, n_lines_min, n_pts_min; lmax_out: int32[n_pairs];
 * stats_out: double[n_pairs][4] = RR, DET, LMEAN, ENTR; smax_out: float[n_pairs]; oti_out:
 * int32[n_pairs]; hist_out: int32[n_pairs][hist_cap], hist_out[p][l] = H[l] for 1 <= l < hist_cap
 * and 0 at l = 0 and beyond min(M, N) (a hist_cap below lmax cuts the copy, not the counts). Every
 * output may be NULL and is then not computed; smax_out NULL skips the S pass. lmin < 1 returns
 * ACOSS_E_ARG, as does hist_out with hist_cap < 1. The line histogram of a pair lives in LDS and
 * takes lines of at most 16,383 cells (16,384 bins, 64 KiB): a stacked length of max_len above that
 * returns ACOSS_E_SHAPE when a line measure is asked for. */
int acoss_crp_rqa(const float* feats, const int64_t* track_off, const int32_t* track_len, int32_t n_tracks,
                  int32_t max_len, const int32_t* pairs, int64_t n_pairs, const acoss_crp_params* params,
                  int32_t lmin, int64_t* counts_out, int32_t* lmax_out, double* stats_out, float* smax_out,
                  int32_t* oti_out, int32_t hist_cap, int32_t* hist_out, void* hip_stream);
/* the same on a given binary matrix (mirrors acoss_align_crp, non-binary input refused alike):
 * counts_out int64[4], lmax_out int32[1], stats_out double[4], smax_out float[1], hist_out
 * int32[hist_cap]. An empty matrix is answered with zeros. min(M, N) above 16,383, or more than
 * 2^31 - 1 cells (a bin is an int32), returns ACOSS_E_SHAPE when a line measure is asked for. */
int acoss_rqa_crp(const uint8_t* crp, int32_t M, int32_t N, int32_t lmin, int64_t* counts_out, int32_t* lmax_out,
                  double* stats_out, float* smax_out, int32_t hist_cap, int32_t* hist_out, void* hip_stream);

/* The seven entries above that make a CRP from chroma, with the binarisation chosen by
 * acoss_crp_params2 (the definition of ACOSS_BIN_OTI is at the struct). Each takes the arguments of
 * the entry it is the twin of, gives its outputs under its conventions and refusals, and with
 * binarize = ACOSS_BIN_PERCENTILE is that entry: the entries without a 2 widen their params with
 * binarize = 0 and run the same driver, kernels and launches. Under ACOSS_BIN_OTI only the mask
 * producer differs: the aligners, the tracing and direction DPs, the backtrack and the line walk
 * consume its words unchanged.
 * acoss_crp_pair2 under ACOSS_BIN_OTI: thr_row and thr_col must be NULL (ACOSS_E_ARG otherwise: there
 * are no thresholds), dist is D_0, crp the mask of the batch kernel, and closer_out (may be NULL)
 * receives closer(i, j) as (Mp x Np) uint8. Under ACOSS_BIN_PERCENTILE closer_out must be NULL. */
int acoss_crp_align2(const float* feats, const int64_t* track_off, const int32_t* track_len, int32_t n_tracks,
                     int32_t max_len, const int32_t* pairs, int64_t n_pairs, const acoss_crp_params2* params,
                     float* qmax_out, float* dmax_out, int32_t* oti_out, void* hip_stream);
int acoss_crp_pair2(const float* X, int32_t M, const float* Y, int32_t N, const acoss_crp_params2* params,
                    float* dist, float* thr_row, float* thr_col, uint8_t* crp, int32_t* oti, uint8_t* closer_out,
                    void* hip_stream);
int acoss_crp_locate2(const float* feats, const int64_t* track_off, const int32_t* track_len, int32_t n_tracks,
                      int32_t max_len, const int32_t* pairs, int64_t n_pairs, const acoss_crp_params2* params,
                      float* qmax_out, int32_t* seg_out, int32_t* oti_out, void* hip_stream);
int acoss_crp_locate_dmax2(const float* feats, const int64_t* track_off, const int32_t* track_len, int32_t n_tracks,
                           int32_t max_len, const int32_t* pairs, int64_t n_pairs, const acoss_crp_params2* params,
                           float* dmax_out, int32_t* seg_out, int32_t* oti_out, void* hip_stream);
int acoss_crp_path2(const float* feats, const int64_t* track_off, const int32_t* track_len, int32_t n_tracks,
                    int32_t max_len, const int32_t* pairs, int64_t n_pairs, const acoss_crp_params2* params,
                    float* qmax_out, int32_t* seg_out, int32_t* oti_out, int32_t path_cap, int32_t* len_out,
                    int32_t* path_out, void* hip_stream);
int acoss_crp_path_dmax2(const float* feats, const int64_t* track_off, const int32_t* track_len, int32_t n_tracks,
                         int32_t max_len, const int32_t* pairs, int64_t n_pairs, const acoss_crp_params2* params,
                         float* dmax_out, int32_t* seg_out, int32_t* oti_out, int32_t path_cap, int32_t* len_out,
                         int32_t* path_out, void* hip_stream);
int acoss_crp_rqa2(const float* feats, const int64_t* track_off, const int32_t* track_len, int32_t n_tracks,
                   int32_t max_len, const int32_t* pairs, int64_t n_pairs, const acoss_crp_params2* params,
                   int32_t lmin, int64_t* counts_out, int32_t* lmax_out, double* stats_out, float* smax_out,
                   int32_t* oti_out, int32_t hist_cap, int32_t* hist_out, void* hip_stream);

/* Ranked OTI: align over the n best transpositions, keep the best (Serra, Serra and Andrzejak 2009
 * compute Qmax for the few most probable transpositions and keep the largest; essentia's oti=True
 * and the entries above apply one index only).
 *
 * The definition, for a pair (query a, reference b) with mean-chroma profiles pq, pr (what
 * k_track_profile writes, oracle.profile):
 *   dot_k, k = 0 .. 11: the float32 chain acc = fmaf(pq[c], pr[(c - k + 12) % 12], acc) for
 *     c = 0 .. 11 from acc = 0: the values the global OTI compares.
 *   order: the twelve shifts sorted by dot_k descending, equal dots keeping the smaller shift first
 *     (a stable sort), built as twelve selections of "the first strict maximum among the shifts not
 *     yet taken". order[0] is the OTI of the entries above, by the same comparisons.
 *   pick r (0 .. 11) applies order[r] wherever the OTI index is applied: the roll of the reference
 *     under ACOSS_BIN_PERCENTILE, g under ACOSS_BIN_OTI. Nothing else changes: the distance is
 *     oracle.crp_dist(X, Y, order[r], m, tau), norms of the un-rolled tracks.
 *   best of n (n_oti = n in 1 .. 12): a score (Qmax, dmax) is the maximum over picks 0 .. n - 1,
 *     folded in pick order with a strict >, so the smallest pick attaining it wins; Qmax and dmax
 *     each keep their own winner.
 * With oti = 0 there is no ranking: n_oti > 1, a nonzero oti_pick or a pick plane then return
 * ACOSS_E_ARG, as do n_oti outside 1 .. 12 and oti_pick outside 0 .. 11. */
typedef struct acoss_crp_params3 {
  acoss_crp_params2 base;
  int32_t n_oti;     /* 1 .. 12, read by acoss_crp_align3 only; the others require 1 */
  int32_t oti_pick;  /* 0 .. 11, applied to every pair when no pick plane is given; acoss_crp_align3 requires 0 */
} acoss_crp_params3;

/* order and dot_k of every pair: shifts_out int32[n_pairs][12] = order, dots_out float[n_pairs][12]
 * = dot_k indexed by the shift k (may be NULL). Device pointers; runs the profile kernel of the
 * aligners and one lane per pair. */
int acoss_oti_ranked(const float* feats, const int64_t* track_off, const int32_t* track_len, int32_t n_tracks,
                     const int32_t* pairs, int64_t n_pairs, int32_t* shifts_out, float* dots_out, void* hip_stream);

/* acoss_crp_align2 with best of n_oti. qmax_out / dmax_out: the best-of-n scores; oti_q_out,
 * oti_d_out: the shifts that won them; pick_q_out, pick_d_out: the winning picks (int32[n_pairs]
 * each). Every output may be NULL; an aligner none of whose three outputs is asked for does not
 * run. Per DP batch (ACOSS_BATCH_PAIRS chunking as before) the order is made once, then each round
 * r < n_oti runs the CRP at pick r, the DPs into a scratch row and a fold into the outputs; the
 * per-track preparation runs once per call. n_oti = 1 makes no order and is acoss_crp_align2 bit
 * for bit (picks 0, both shifts its oti_out). */
int acoss_crp_align3(const float* feats, const int64_t* track_off, const int32_t* track_len, int32_t n_tracks,
                     int32_t max_len, const int32_t* pairs, int64_t n_pairs, const acoss_crp_params3* params,
                     float* qmax_out, float* dmax_out, int32_t* oti_q_out, int32_t* oti_d_out, int32_t* pick_q_out,
                     int32_t* pick_d_out, void* hip_stream);
/* acoss_crp_pair2 at the scalar pick params->oti_pick: dist, thr_row, thr_col, crp, closer_out and
 * oti are those of the transposition order[oti_pick]. n_oti must be 1. */
int acoss_crp_pair3(const float* X, int32_t M, const float* Y, int32_t N, const acoss_crp_params3* params,
                    float* dist, float* thr_row, float* thr_col, uint8_t* crp, int32_t* oti, uint8_t* closer_out,
                    void* hip_stream);
/* The entries ending in 2 with one more argument: picks, device int32[n_pairs], the pick of every
 * pair; NULL means params->oti_pick for every pair. oti_out is the shift applied. n_oti must be 1.
 * A pick outside 0 .. 11 in the plane returns ACOSS_E_ARG after the call has run (a device flag read
 * back; that pair ran at pick 0): these entries then synchronise the stream once. With oti_pick = 0
 * and picks = NULL each is its twin ending in 2, bit for bit. */
int acoss_crp_locate3(const float* feats, const int64_t* track_off, const int32_t* track_len, int32_t n_tracks,
                      int32_t max_len, const int32_t* pairs, int64_t n_pairs, const acoss_crp_params3* params,
                      float* qmax_out, int32_t* seg_out, int32_t* oti_out, const int32_t* picks, void* hip_stream);
int acoss_crp_locate_dmax3(const float* feats, const int64_t* track_off, const int32_t* track_len, int32_t n_tracks,
                           int32_t max_len, const int32_t* pairs, int64_t n_pairs, const acoss_crp_params3* params,
                           float* dmax_out, int32_t* seg_out, int32_t* oti_out, const int32_t* picks,
                           void* hip_stream);
int acoss_crp_path3(const float* feats, const int64_t* track_off, const int32_t* track_len, int32_t n_tracks,
                    int32_t max_len, const int32_t* pairs, int64_t n_pairs, const acoss_crp_params3* params,
                    float* qmax_out, int32_t* seg_out, int32_t* oti_out, int32_t path_cap, int32_t* len_out,
                    int32_t* path_out, const int32_t* picks, void* hip_stream);
int acoss_crp_path_dmax3(const float* feats, const int64_t* track_off, const int32_t* track_len, int32_t n_tracks,
                         int32_t max_len, const int32_t* pairs, int64_t n_pairs, const acoss_crp_params3* params,
                         float* dmax_out, int32_t* seg_out, int32_t* oti_out, int32_t path_cap, int32_t* len_out,
                         int32_t* path_out, const int32_t* picks, void* hip_stream);
int acoss_crp_rqa3(const float* feats, const int64_t* track_off, const int32_t* track_len, int32_t n_tracks,
                   int32_t max_len, const int32_t* pairs, int64_t n_pairs, const acoss_crp_params3* params,
                   int32_t lmin, int64_t* counts_out, int32_t* lmax_out, double* stats_out, float* smax_out,
                   int32_t* oti_out, int32_t hist_cap, int32_t* hist_out, const int32_t* picks, void* hip_stream);

/* acoss smith_waterman_constrained (A8, acoss/algorithms/utils/alignment_tools.py:25-46) on
 * a batch of binary matrices: matrix b is (rows[b] x cols[b]) uint8 at byte offset off[b]
 * of `mats`. score_out: double[n_mats]. Bit-exact float64 (same evaluation order). */
int acoss_sw_constrained(const uint8_t* mats, const int64_t* off, const int32_t* rows, const int32_t* cols,
                         int32_t n_mats, int32_t max_rows, int32_t max_cols, double* score_out, void* hip_stream);

/* WHERE the constrained Smith-Waterman alignment lies: acoss_sw_constrained with, per matrix, the
 * first and last cell of the alignment behind the score (acoss_sw_locate) or every cell of it
 * (acoss_sw_path). The reference fills a whole score matrix and returns only its maximum; here the
 * tracing DP carries the cell where each path began beside every score and writes no matrix, and
 * the direction DP leaves a 2-bit predecessor code per cell in a workspace plane of about M N / 4
 * bytes per matrix that a second kernel walks back (sw.hip k_swt, k_sw_backtrack). Inputs as
 * acoss_sw_constrained. score_out: double[n_mats], may be NULL, acoss_sw_constrained's bit for bit.
 * seg_out: int32[4 n_mats] = (r0, c0, r1, c1) per matrix (may be NULL for acoss_sw_path). len_out:
 * int32[n_mats]; path_out: int32[n_mats][path_cap][2], the path's cells (r, c) first to last, the
 * rest -1.
 *
 * The definition. B is the binary M x N matrix, S the score matrix of oracle/crp_oracle.cpp
 * or_sw_constrained, all arithmetic float64. Cells are named in B's own coordinates: the
 * reference's score_matrix[i][j] is the cell X = (i - 1, j - 1) here.
 *   scored cells: 2 <= r <= M - 2 and 2 <= c <= N - 2, the reference's loop bounds; every other
 *     cell holds 0.
 *   m(X) = +1 if B[X] else -1; pen(P) = 0 if B[P] else -0.7.
 *   predecessors of X = (r, c), in this fixed order:
 *     a: P = (r-1, c-1)     b: P = (r-2, c-1)     c: P = (r-1, c-2)
 *   each with the value x_k = (S[P_k] + m(X)) + pen(P_k), in exactly that association.
 *   score of a cell: S[X] = max(x_a, x_b, x_c, 0).
 *   chosen predecessor: the FIRST of a, b, c attaining the maximum (a strictly greater value
 *     replaces, an equal one does not). A cell with S[X] == 0 has none; a cell whose chosen
 *     predecessor has S[P] == 0 begins a path, and P is not on the path.
 *   score = max S; end cell: the first cell in row-major order holding it (the reference's > keeps
 *     the first).
 *   path: from the end cell follow chosen predecessors while S[P] > 0; reported origin to end.
 *     Strictly increasing in r and c, steps (1, 1), (2, 1) and (1, 2); every cell lies in
 *     [2, M-2] x [2, N-2] and has S > 0; misses may lie on it (the gaps the -1 paid for); at most
 *     max(0, min(M, N) - 3) cells.
 *   segment: (r0, c0, r1, c1) = (origin, end); (-1, -1, -1, -1) and an empty path where the score
 *     is 0, always so for M < 4 or N < 4.
 *   check of a path: re-accumulating x along it, from 0 at the origin's chosen predecessor,
 *     reproduces the score bit for bit.
 * path_cap below max(1, min(max_rows, max_cols) - 3) returns ACOSS_E_ARG, the message naming the
 * bound; a byte other than 0 / 1 ACOSS_E_NONBINARY; max_rows or max_cols above 65,535
 * ACOSS_E_SHAPE (a cell is packed into 16 + 16 bits). */
int acoss_sw_locate(const uint8_t* mats, const int64_t* off, const int32_t* rows, const int32_t* cols, int32_t n_mats,
                    int32_t max_rows, int32_t max_cols, double* score_out, int32_t* seg_out, void* hip_stream);
int acoss_sw_path(const uint8_t* mats, const int64_t* off, const int32_t* rows, const int32_t* cols, int32_t n_mats,
                  int32_t max_rows, int32_t max_cols, double* score_out, int32_t* seg_out, int32_t path_cap,
                  int32_t* len_out, int32_t* path_out, void* hip_stream);

/* Cross-similarity matrices (A5/A6/A2): acoss get_csm / get_csm_cosine
 * (cross_recurrence.py:30-73), optionally after get_csm_blocked_oti's query rotation
 * (:105-134): with oti_shift >= 0 every 12-bin block of each X row is rolled by oti_shift
 * (np.roll on the chroma axis) first. X (M x d), Y (N x d) float32; out (M x N) float32.
 * kind = 0 euclidean, 1 cosine, 2 self-similarity of X (get_ssm :10-28; Y ignored). */
int acoss_csm(const float* X, int32_t M, const float* Y, int32_t N, int32_t d, int32_t kind, int32_t oti_shift,
              float* out, void* hip_stream);

/* acoss get_oti (cross_recurrence.py:75-103) for a batch: C1, C2 (n x 12) float32 global
 * chroma vectors; out int32[n] = argmax_i sum(roll(C1[k], i) * C2[k]), first max wins. */
int acoss_get_oti(const float* C1, const float* C2, int32_t n, int32_t* out, void* hip_stream);

/* acoss csm_to_binary (A7, cross_recurrence.py:136-161): row-wise kappa nearest neighbours.
 * D (M x N) float32 -> B (M x N) uint8. nneighbs = number of ones per row (the host computes
 * int(np.round(kappa * N)) or kappa itself, as the reference does); nneighbs <= 0 -> all ones.
 * Among equal distances the lowest column index wins (numpy's argpartition choice is
 * arbitrary). */
int acoss_binarize_rows(const float* D, int32_t M, int32_t N, int32_t nneighbs, uint8_t* B, void* hip_stream);

/* acoss getWCSM (A14, similarity_fusion.py:38-54): W = exp(-CSM^2 / (2 (mu*Eps)^2)) with
 * Eps = (rowmean_k2 + colmean_k1 + CSM)/3 of the k2 / k1 smallest per row / column.
 * CSM, W: (M x N) float32. The means add the k smallest in ascending order and exp is the
 * canonical canon_expf, so W equals the CPU oracle's (oracle/ef_oracle.cpp or_ef_wcsm) bit for bit. */
int acoss_wcsm(const float* CSM, int32_t M, int32_t N, int32_t k1, int32_t k2, float mu, float* W,
               void* hip_stream);

/* out[i] = exp(-x[i]) for n float32 values, in the canonical float32 exp shared with the CPU oracle
 * (common.hpp canon_expf): EarlyFusion's early matrix np.exp(-WCSM_sum)
 * (earlyfusion_traile.py:182) for the per-pair path (EarlyFusion.pair_matrices); the batched
 * acoss_earlyfusion applies the same exp inside. out may alias x. */
int acoss_neg_exp(const float* x, int64_t n, float* out, void* hip_stream);

/* One cross-diffusion step of similarity network fusion for matrix `skip` (f2, replaces the body
 * of the loop at acoss/algorithms/utils/similarity_fusion.py:163-174 in doSimilarityFusionWs):
 *   out = S . A . S^T + reg_diag * I,  A = (sum_{m != skip} mats[m]) / (n_mats - 1),
 * S the kNN-truncated row-normalised affinity (getS, :121-143) given as J (n x K) int32 column
 * indices and V (n x K) float64 values, any order within a row (sums run in ascending column
 * order, as scipy's csr product). Every J entry must lie in [0, n) and no column may repeat
 * within a row (scipy's coo -> csr would merge repeats into one term): otherwise ACOSS_E_ARG,
 * checked on the device before any product runs. mats: HOST array of n_mats device pointers
 * to (n x n) float64 matrices; out (n x n) float64 may alias mats[skip] but no other.
 * n_mats >= 2 (any number; more than 16 others are averaged in passes), 0 < K <= min(n, 64).
 * validate = 1: the index check synchronises the stream once and a bad J returns ACOSS_E_ARG;
 * validate = 0 (J already checked, e.g. once per fusion): no sync, and a bad row is replaced by
 * a weight-0 entry on its own column, so no kernel reads outside the matrices. */
int acoss_snf_step(const double* const* mats, int32_t n_mats, int32_t skip, int32_t n, const int32_t* J,
                   const double* V, int32_t K, double reg_diag, double* out, int32_t validate, void* hip_stream);

/* The same step split at its one exchange point, for a fusion row-sharded across ranks (SURVEY
 * §8f row 2: each rank owns rows [row0, row0 + rows) of every matrix; the same loop body,
 * similarity_fusion.py:163-174). Both halves are bit-identical to the matching rows of
 * acoss_snf_step: same kernels, same summation order.
 *   acoss_snf_diffuse_rows: B_rows = rows [row0, row0 + rows) of B = A . S^T, from the (rows x n)
 *     stripes mats[m] of the matrices (HOST array of device pointers); B_rows (rows x n) may
 *     overlap mats[skip] but no other stripe.
 *   (the caller all-gathers the stripes of B into the whole (n x n) B)
 *   acoss_snf_left_rows: out = rows [row0, row0 + rows) of S . B + reg_diag * I, from the whole
 *     (n x n) B; out (rows x n) must not overlap B.
 * J, V, K, validate as for acoss_snf_step (J, V describe all n rows of S in both calls). */
int acoss_snf_diffuse_rows(const double* const* mats, int32_t n_mats, int32_t skip, int32_t n, int32_t rows,
                           const int32_t* J, const double* V, int32_t K, double* B_rows, int32_t validate,
                           void* hip_stream);
int acoss_snf_left_rows(const double* B, int32_t n, int32_t row0, int32_t rows, const int32_t* J, const double* V,
                        int32_t K, double reg_diag, double* out, int32_t validate, void* hip_stream);

/* SiMPle matrix profile score (A11, acoss/algorithms/simple_silva.py:68-118) for a batch of
 * ordered pairs, including the per-pair OTI roll of the reference (Simple.oti, :45-54).
 * feats: packed (12 x n_t) float64 blocks, track t at element offset track_off[t] (dim-major,
 * as the reference's seq arrays). score_out[p] = median_i min_j dist (the reference stores
 * -score, simple_silva.py:125). apply_oti = 0 scores the reference as given (Simple.simple_sim
 * alone); oti_out (may be NULL) always receives the Simple.oti index. */
int acoss_simple_mp(const double* feats, const int64_t* track_off, const int32_t* track_len, int32_t n_tracks,
                    int32_t max_len, const int32_t* pairs, int64_t n_pairs, int32_t sslen, int32_t apply_oti,
                    double* score_out, int32_t* oti_out, void* hip_stream);

/* The SiMPle matrix profile itself and its index (Silva et al., ISMIR 2016): for every length-sslen
 * subsequence of the query its distance to the nearest subsequence of the reference, and which
 * one that is. Inputs and refusals as acoss_simple_mp (sslen in 1..16, ACOSS_E_ARG otherwise;
 * max_len above 4096 returns ACOSS_E_SHAPE). For pair p = (a, b): P = len[a] - sslen + 1 rows,
 * Q = len[b] - sslen + 1 columns. The profiles are ragged, not padded (their lengths are known
 * before the call): pair p's occupies mp_out[prof_off[p] .. prof_off[p] + max(P, 0)) and the same
 * range of mpi_out.
 *
 * The definition.
 *   dist(i, j) is the canonical value of oracle/crp_oracle.cpp or_simple_sim, on the reference
 *     rolled by the OTI index when apply_oti is set: a frame dot is the product of bin 0 followed by
 *     the fma chain over the reference's own bins 1..11, frame norms likewise, window sums are
 *     sequential adds over t = 0..sslen-1, dist = (sb[j] + sa[i]) - 2 qt.
 *   mp[i] = min_j dist(i, j): the row minimum the score kernels form, bit for bit.
 *   mpi[i] = the smallest j with dist(i, j) == mp[i] (an IEEE compare: the oracle loop's
 *     `dist < mn` keeps the first of equal distances).
 *   A row with no distance below +inf (NaN features under its window, or Q <= 0 while P > 0)
 *     holds NaN in mp and -1 in mpi.
 *   score_out[p] (may be NULL) = median(mp), acoss_simple_mp's score_out[p] bit for bit (NaN where
 *     P <= 0 or Q <= 0); oti_out[p] (may be NULL) = acoss_simple_mp's.
 * A pair's output does not depend on its place in the list; a pair listed twice fills both of its
 * ranges identically.
 *
 * prof_off: device int64[n_pairs + 1], checked on the device before any profile write: for every
 * pair prof_off[p] >= 0, prof_off[p] + max(P, 0) <= prof_off[p + 1] and prof_off[p + 1] <=
 * prof_total (the element count of mp_out and of mpi_out). Otherwise ACOSS_E_ARG, the message
 * naming the first such pair, and nothing is written. (The check rides on the stream
 * synchronisation acoss_simple_mp has as well.)
 * Kernels (simple.hip): k_simple_mfma<1> for sslen = 10 at every length, k_simple_pair<1> for every
 * other sslen; each walks the pair twice, the second time comparing every distance with its row's
 * minimum. The ACOSS_SIMPLE_K / SH / PPB / RED / MFMA overrides do not apply; a launch takes up to
 * 2^20 pairs, or ACOSS_SIMPLE_PROFILE_BATCH pairs if that is set lower. */
int acoss_simple_profile(const double* feats, const int64_t* track_off, const int32_t* track_len, int32_t n_tracks,
                         int32_t max_len, const int32_t* pairs, int64_t n_pairs, int32_t sslen, int32_t apply_oti,
                         const int64_t* prof_off, int64_t prof_total, double* mp_out, int32_t* mpi_out,
                         double* score_out, int32_t* oti_out, void* hip_stream);

/* The SiMPle self-join (Silva et al., ISMIR 2016: the other of the paper's "subsequences joins"):
 * the matrix profile of a track against itself with the trivial matches excluded, its motif (the
 * repeated section) and its discord (the most unusual passage). feats, track_off, track_len,
 * n_tracks and max_len as acoss_simple_profile; tracks: device int32[n_sel], the tracks to profile.
 * Entry e, track t = tracks[e] of n columns, P = n - sslen + 1: its P rows (none when P <= 0) occupy
 * mp_out[prof_off[e] .. prof_off[e] + max(P, 0)) and the same range of mpi_out.
 *
 * The definition.
 *   dist(i, j), 0 <= i, j < P, is acoss_simple_profile's canonical distance with query = reference
 *     = t and no roll (k = 0): a frame dot is the product of bin 0 followed by the fma chain over
 *     bins 1..11, frame norms likewise, window sums are sequential adds over t = 0..sslen-1,
 *     dist = (s[j] + s[i]) - 2 qt. (dist(i, j) == dist(j, i) bit for bit, and dist(i, i) == 0.)
 *   mp[i] = the minimum of dist(i, j) over the j with |i - j| > excl; mpi[i] = the smallest such j
 *     attaining it (an IEEE compare, the first of equals).
 *   A row with no admissible distance below +inf holds NaN in mp and -1 in mpi: every row when
 *     P - 1 <= excl, and rows with NaN features under their window.
 *   motif_out[2 e .. 2 e + 2) (may be NULL) = (i*, mpi[i*]), i* the smallest row attaining the
 *     minimum of mp over its rows that are not NaN; discord_out[e] (may be NULL) = the smallest row
 *     attaining their maximum. Without such a row (-1, -1) and -1.
 * An entry's output does not depend on its place in the list; a track listed twice fills both of
 * its ranges identically. No median and no OTI are formed.
 *
 * Refusals as acoss_simple_profile (sslen outside 1..16: ACOSS_E_ARG; max_len above 4096:
 * ACOSS_E_SHAPE; prof_off, device int64[n_sel + 1], checked on the device before any write, the
 * message naming the first bad entry); in addition excl < 0 or a track index outside
 * [0, n_tracks) (checked on the device as well, the message naming the first such entry) returns
 * ACOSS_E_ARG. Nothing is written in any of these cases.
 * Kernels (simple.hip): the SELF instantiations k_simple_mfma<1, 1> (sslen = 10, every length) and
 * k_simple_pair<1, 1> (every other sslen) of the profile kernels, then k_simple_motif, one block per
 * entry. ACOSS_SIMPLE_PROFILE_BATCH applies as in acoss_simple_profile. */
int acoss_simple_self_profile(const double* feats, const int64_t* track_off, const int32_t* track_len,
                              int32_t n_tracks, int32_t max_len, const int32_t* tracks, int64_t n_sel, int32_t sslen,
                              int32_t excl, const int64_t* prof_off, int64_t prof_total, double* mp_out,
                              int32_t* mpi_out, int32_t* motif_out, int32_t* discord_out, void* hip_stream);

/* Per-track median downsampling of chroma (A13: Serra09/ChenFusion.load_features,
 * acoss/algorithms/rqa_serra09.py:44-53 and latefusion_chen.py:46-56, which call
 * librosa.util.sync(chroma.T, arange(0, n, factor), aggregate=np.median)).
 * feats: packed (sum n, 12) float32, track t at frame offset track_off[t]; max_len = max n.
 * out: track t's ceil(n_t / factor) x 12 float32 rows at frame offset out_off[t].
 * factor <= 64. */
int acoss_median_downsample(const float* feats, const int64_t* track_off, const int32_t* track_len, int32_t n_tracks,
                            int32_t max_len, int32_t factor, float* out, const int64_t* out_off, void* hip_stream);

/* Per-track SiMPle features (A12: Simple.load_features + Simple.smooth,
 * acoss/algorithms/simple_silva.py:34-43,56-66): window means (win=200, hop skip=100) ->
 * 'same' zero-filled convolution with the host weights smooth[0..smooth_len) (normalised
 * symmetric Hann(6) in the reference) -> per-column L2 normalisation.
 * out: track t's (12 x floor(n_t / skip)) float64 block (dim-major) at element offset
 * out_off[t]; out_elems = total doubles in out. smooth is a HOST pointer. */
int acoss_simple_features(const float* feats, const int64_t* track_off, const int32_t* track_len, int32_t n_tracks,
                          int32_t win, int32_t skip, const double* smooth, int32_t smooth_len, double* out,
                          const int64_t* out_off, int64_t out_elems, void* hip_stream);

/* FTM2D shingles (FTM2D.load_features, acoss/algorithms/ftm2d.py:52-66, with chrompwr :100-117 and
 * btchroma_to_fftmat :120-138) for a batch of tracks. feats: packed (sum n, 12) float32 chroma as
 * above; max_len = max n. bounds: every track's segment boundaries, int64 frame indices, sorted,
 * unique and clipped to [0, n_t] (np.unique(concat([0], clip(onsets, 0, n), [n])), what
 * librosa.util.sync(hpcp.T, onsets) slices at, :58); track t's are bounds[bound_off[t] ..
 * bound_off[t + 1]), bound_off int64[n_tracks + 1] with bound_off[0] = 0, so the track has
 * bound_off[t + 1] - bound_off[t] - 1 beats. Per track: the float32 median of every (segment, bin)
 * exactly as np.median, chrompwr(., pwr), |fft2| of every 12 x win window fftshift-ed and flattened
 * row-major, each window divided by its L2 norm (0 -> 1) and mapped by log(C x + 1), the
 * per-coefficient median over the windows, divided by the L2 norm of the medians (NaN for an
 * all-silent track, as the reference's 0 / 0); float64 from chrompwr on.
 * shingles_out: (n_tracks x 12 win) float64. win must be 75 (ACOSS_E_ARG otherwise): the twiddle
 * matrix' size is a compile-time constant. A track with fewer than win beats or more than 4170
 * (4096 windows) returns ACOSS_E_SHAPE, the message naming the track index; the offsets are read
 * back from the device for that check, which synchronises the stream once. */
int acoss_ftm2d_shingles(const float* feats, const int64_t* track_off, const int32_t* track_len, int32_t n_tracks,
                         int32_t max_len, const int64_t* bounds, const int64_t* bound_off, int32_t win, double pwr,
                         double C, double* shingles_out, void* hip_stream);

/* The first two steps of acoss_ftm2d_shingles alone, for parity tests (ftm2d.py:58-59, 100-117):
 * track t's beat-synchronous medians (sync_out, float32, may be NULL) and their chrompwr (chroma_out,
 * float64) as (12 x beats) blocks at element offset 12 (bound_off[t] - t). max_beats = the largest
 * beat count (host scalar); any segment length is accepted. */
int acoss_ftm2d_beatsync(const float* feats, const int64_t* track_off, const int32_t* track_len, int32_t n_tracks,
                         const int64_t* bounds, const int64_t* bound_off, int32_t max_beats, double pwr,
                         float* sync_out, double* chroma_out, void* hip_stream);

/* FTM2D pair scores (FTM2D.similarity, ftm2d.py:85-97): scores_out[p] = exp(-sum_d (s_i[d] - s_j[d])^2)
 * for (i, j) = (pairs[2p], pairs[2p+1]), float64, the squared differences summed directly in one
 * fixed order (a pair's score does not depend on its place in the list; (i, i) scores exactly 1).
 * shingles: (n_tracks x dim) float64, dim <= 1024 (900 for acoss_ftm2d_shingles' output). A pair
 * naming a track outside [0, n_tracks) scores NaN. */
int acoss_ftm2d_scores(const double* shingles, int32_t n_tracks, int32_t dim, const int32_t* pairs, int64_t n_pairs,
                       double* scores_out, void* hip_stream);

/* FTM2D shortlist: for query row q of q_shingles (n_q x dim) the k rows j of r_shingles (n_r x dim)
 * of largest score exp(-sum_d (s_q[d] - s_j[d])^2), in decreasing score order, equal scores by
 * increasing j: idx_out[q] = np.argsort(-row, kind="stable")[:k] of the score row, score_out[q] the
 * scores, each bit for bit what acoss_ftm2d_scores returns for that pair (same summation order).
 * The n_q x n_r scores are never stored: the k best of a query live in LDS while its wave walks
 * over the reference rows (with few queries the rows are split into up to 16 ranges whose partial
 * lists, n_q x ranges x k entries of workspace, are merged by a second kernel). self_off >= 0: query q is reference row self_off + q, which is left
 * out (a rank passes its row stripe as the queries and its first row as self_off); -1: nothing is
 * left out. A pair whose score is NaN is never listed; slots left over (fewer than k candidates,
 * or a NaN query row) hold idx -1 and score NaN. idx_out int32, score_out float64, both (n_q x k).
 * dim in [1, 1024], k in [1, 1024] (ACOSS_E_ARG otherwise); the two tables may be the same buffer. */
int acoss_ftm2d_topk(const double* q_shingles, int32_t n_q, const double* r_shingles, int32_t n_r, int32_t dim,
                     int32_t self_off, int32_t k, int32_t* idx_out /* n_q x k */, double* score_out /* n_q x k */,
                     void* hip_stream);

/* Batched EarlyFusion scores (A15: EarlyFusion.similarity, acoss/algorithms/earlyfusion_traile.py:157-198).
 * Block features of every track packed row-major: mfcc (sum nb x d_mfcc), ssm (sum nb x d_ssm),
 * chroma (sum nb x d_chroma, 12-bin blocks) float32, track t's rows at block_off[t], n_blocks[t]
 * of them; chroma_med (n_tracks x 12) float32. For every pair: CSMs (euclid, euclid, blocked-OTI
 * cosine), csm_to_binary(kappa), getWCSM(K, K, mu) fusion, and smith_waterman_constrained of the
 * four binary matrices -> scores_out[4 p + {0: mfccs, 1: ssms, 2: chromas, 3: early}] (float64).
 * Pairs are processed in the order given; for large lists, order them (reference band, query) as
 * acoss/_lib.py earlyfusion does (1.24x at 15,000 Da-TACOS-shaped songs): a band of reference
 * tracks' rows then stays cached while the query rows stream past. */
int acoss_earlyfusion(const float* mfcc, const float* ssm, const float* chroma, const float* chroma_med,
                      const int64_t* block_off, const int32_t* n_blocks, int32_t n_tracks, int32_t max_blocks,
                      int32_t d_mfcc, int32_t d_ssm, int32_t d_chroma, const int32_t* pairs, int64_t n_pairs,
                      double kappa, int32_t K, float mu, double* scores_out, void* hip_stream);

/* acoss_earlyfusion with WHERE each of the four alignments lies: the same stages up to the four
 * binary matrices of every pair (rows: the query's blocks, columns: the reference's), then
 * acoss_sw_locate's or acoss_sw_path's kernels over them (the definition is there). Arguments as
 * acoss_earlyfusion; scores_out: double[4 n_pairs], acoss_earlyfusion's bit for bit. seg_out:
 * int32[n_pairs][4][4] = (r0, c0, r1, c1) of matrix s (mfccs, ssms, chromas, early) of pair p, in
 * blocks (may be NULL for the path entry); len_out: int32[n_pairs][4]; path_out:
 * int32[n_pairs][4][path_cap][2], padded with -1. path_cap below max(1, max_blocks - 3) returns
 * ACOSS_E_ARG, the message naming the bound. The direction planes (about ld^2 bytes per pair for
 * the four matrices) enter the per-pair chunk size of the path entry only. */
int acoss_earlyfusion_locate(const float* mfcc, const float* ssm, const float* chroma, const float* chroma_med,
                             const int64_t* block_off, const int32_t* n_blocks, int32_t n_tracks, int32_t max_blocks,
                             int32_t d_mfcc, int32_t d_ssm, int32_t d_chroma, const int32_t* pairs, int64_t n_pairs,
                             double kappa, int32_t K, float mu, double* scores_out, int32_t* seg_out,
                             void* hip_stream);
int acoss_earlyfusion_path(const float* mfcc, const float* ssm, const float* chroma, const float* chroma_med,
                           const int64_t* block_off, const int32_t* n_blocks, int32_t n_tracks, int32_t max_blocks,
                           int32_t d_mfcc, int32_t d_ssm, int32_t d_chroma, const int32_t* pairs, int64_t n_pairs,
                           double kappa, int32_t K, float mu, double* scores_out, int32_t* seg_out, int32_t path_cap,
                           int32_t* len_out, int32_t* path_out, void* hip_stream);

/* EarlyFusion's per-pair similarity network fusion ("early SNF", Tralie 2017: the early fusion of
 * the paper, which EarlyFusion.similarity's `early` score shortcuts) for a batch of pairs. Bank and
 * pair arguments as acoss_earlyfusion. Pair p = (a, b), M and N blocks, n = M + N:
 *  1. For each feature f in the order mfccs, ssms, chromas: CSM_f (M x N, float32) is the matrix
 *     acoss_earlyfusion forms (euclid, euclid, blocked-OTI cosine); SSMA_f (M x M) and SSMB_f
 *     (N x N) are the same distance of a track's blocks against themselves with no roll (get_ssm /
 *     get_csm_cosine(X, X); the same kernels as CSM_f, once per track of a chunk).
 *  2. W_f = getWCSMSSM(SSMA_f, SSMB_f, CSM_f, K, mu) (similarity_fusion.py:76-99): k1 =
 *     int(K M / (M + N)), k2 = K - k1; all float32 (numpy's dtype rule), every exp the canonical
 *     canon_expf. The CSM block is acoss_wcsm(CSM_f, k1, k2, mu). The SSM blocks follow getW
 *     (:15-36) with k = k1 (A) or k2 (B): DSym = 0.5 (D + D^T) with a zero diagonal; MeanDist = the
 *     mean of the k + 1 smallest of each row, added in ascending order, times (k + 1), over k;
 *     Eps = ((MeanDist_i + MeanDist_j) + DSym) / 3; Denom = 2 (mu Eps)^2, a zero replaced by 1;
 *     W = exp(-DSym^2 / Denom). The parent [[W_A, W_AB], [W_AB^T, W_B]] is float64 and holds the
 *     float32 values exactly.
 *  3. F = doSimilarityFusionWs([W_mfccs, W_ssms, W_chromas], K, niters, reg_diag) (:146-186), all
 *     float64: getP divides each row by its sum (columns added in ascending order; a zero sum is
 *     replaced by 1); getS keeps the K largest of each row of W, self included, the lowest column
 *     among equal values, divided by their sum (added in ascending column order; zero -> 1). A step
 *     for matrix i is S_i ((sum of the other two) / 2) S_i^T + reg_diag I (reg_diag > 0), both
 *     products summed over the K neighbours in ascending column order from +0, one rounded
 *     multiply and add per term. The first round reads the three P only; from the second round on
 *     matrix i sees the new matrices k < i (the reference's `Pts = nextPts` aliasing). F is
 *     (((0 + P_0) + P_1) + P_2) / 3; niters = 0 gives the mean of the three P.
 *  4. cross = F[:M, M:] + F[M:, :M]^T (M x N). The binary matrix has nn ones per row at the nn
 *     LARGEST values of cross, ties to the lowest column, nn = csm_to_binary's count for kappa and
 *     N: csm_to_binary(exp(-cross), kappa) up to where a float64 exp merges two values.
 *     score_out[p] = smith_waterman_constrained of that matrix: acoss_sw_constrained's bits.
 * A pair the reference cannot fuse (it raises) breaks 1 <= k1 <= M - 2, 1 <= k2 <= N - 2 or K < n:
 * it scores NaN and writes NaN over its range of cross_out; the other pairs are untouched and the
 * call returns ACOSS_OK.
 * score_out: double[n_pairs]. cross_out: NULL, or pair p's M x N matrix, row-major, at
 * cross_out[cross_off[p] ..); cross_off: int64[n_pairs + 1], checked on the device before any
 * write (negative, shorter than M N, or past cross_total: ACOSS_E_ARG naming the first bad pair).
 * K: 1 <= K <= 64 whatever max_blocks is (acoss_earlyfusion's K <= max_blocks does not apply: K is
 * weighed against each pair's own M and N by the three conditions above, so K = 50 on a bank of
 * 47-block tracks fuses every pair that meets them).
 * ACOSS_E_ARG as acoss_earlyfusion but for that K rule, and for niters < 0, reg_diag < 0, K > 64, a
 * track of more than 512 blocks or a pair naming a track outside [0, n_tracks). Pairs with
 * n <= 101 run all their 3 niters steps in one workgroup with two n x n float64 matrices in LDS
 * (16 n^2 <= 160 KB);
 * longer ones keep their matrices in the workspace, chunked under ACOSS_EF_BYTES. The operations
 * and their order are the same in both, so a pair's output depends neither on its place in the
 * list nor on the chunking; a pair listed twice gives the same bits twice. */
int acoss_earlyfusion_snf(const float* mfcc, const float* ssm, const float* chroma, const float* chroma_med,
                          const int64_t* block_off, const int32_t* n_blocks, int32_t n_tracks, int32_t max_blocks,
                          int32_t d_mfcc, int32_t d_ssm, int32_t d_chroma, const int32_t* pairs, int64_t n_pairs,
                          double kappa, int32_t K, float mu, int32_t niters, double reg_diag, double* score_out,
                          const int64_t* cross_off, int64_t cross_total, double* cross_out, void* hip_stream);

/* ---------------------------------------------------------------------------------
 * EarlyFusion's binarisation by MUTUAL nearest neighbours (Tralie 2017, "Early MFCC and HPCP fusion
 * for robust cover song identification"; the author's CSMToBinaryMutual = CSMToBinary(D) *
 * CSMToBinary(D.T).T). The reference's csm_to_binary keeps the row half only (SURVEY.md appendix,
 * defect 7), and that stays the default of every entry: ACOSS_EF_BIN_ROWS gives the twin's bits.
 *
 * "mutual": for a float32 M x N matrix D and kappa,
 *   count(kappa, n) = int(np.round(kappa * n)) for kappa < 1 (float64 product, half to even: C rint;
 *     at kappa = 0.1: 0 for n = 5, 2 for n = 15, 2 for n = 25), else int(kappa); the C ABI clamps a
 *     count to its line length, min(count, n), as the row kernels always have. nn_r = count(kappa,
 *     N), nn_c = count(kappa, M). kappa == 0 gives all ones.
 *   Row rule:    R(i, j) = 1 iff fewer than nn_r cells of row i come before (i, j) in the order
 *     (value ascending, column ascending): csm_to_binary with ties to the lowest column, what every
 *     entry computes today.
 *   Column rule: C(i, j) = 1 iff fewer than nn_c cells of column j come before (i, j) in the order
 *     (value ascending, ROW ascending). The order on values is the row rule's (the float's bit
 *     pattern mapped to an unsigned key, so -0 < +0), hence C(D) = R(D^T)^T bit for bit.
 *   B = R & C.
 * So B is a subset of R; row sums are at most nn_r and column sums at most nn_c; mutual(D^T) =
 * mutual(D)^T exactly; for count-valued kappa the masks are nested in kappa. A short query against
 * a long reference can have nn_c == 0 (M = 4, N = 30, kappa = 0.1: nn_r = 3, nn_c = 0): the mask is
 * empty and the score 0, by definition.
 * Early SNF: the matrix is the float64 cross block and both rules take the LARGEST values: R the
 * nn_r largest of each row, ties to the lowest column (today's rule), C the nn_c largest of each
 * column, ties to the lowest row (-0 == +0), B = R & C. A pair the reference cannot fuse keeps its
 * NaN score and an empty matrix.
 * The Python layer raises the reference's "kth(=%d) out of bounds (%d)" for nn_r >= N and, under
 * mutual, for nn_c >= M; the C ABI clamps and does not raise. */
#define ACOSS_EF_BIN_ROWS 0
#define ACOSS_EF_BIN_MUTUAL 1

/* acoss_earlyfusion, acoss_earlyfusion_locate and acoss_earlyfusion_path with `binarize` (one of
 * the two values above; anything else: ACOSS_E_ARG) directly after mu; everything else as the
 * twin, which forwards here with ACOSS_EF_BIN_ROWS. Under ACOSS_EF_BIN_MUTUAL the column pass
 * (csrc/ef_binarize.hip) runs after each row-binarise launch, over the three CSM planes before the
 * fusion overwrites the first, and over the early matrix; with ACOSS_EF_BIN_ROWS nothing new runs. */
int acoss_earlyfusion2(const float* mfcc, const float* ssm, const float* chroma, const float* chroma_med,
                       const int64_t* block_off, const int32_t* n_blocks, int32_t n_tracks, int32_t max_blocks,
                       int32_t d_mfcc, int32_t d_ssm, int32_t d_chroma, const int32_t* pairs, int64_t n_pairs,
                       double kappa, int32_t K, float mu, int32_t binarize, double* scores_out, void* hip_stream);
int acoss_earlyfusion_locate2(const float* mfcc, const float* ssm, const float* chroma, const float* chroma_med,
                              const int64_t* block_off, const int32_t* n_blocks, int32_t n_tracks, int32_t max_blocks,
                              int32_t d_mfcc, int32_t d_ssm, int32_t d_chroma, const int32_t* pairs, int64_t n_pairs,
                              double kappa, int32_t K, float mu, int32_t binarize, double* scores_out,
                              int32_t* seg_out, void* hip_stream);
int acoss_earlyfusion_path2(const float* mfcc, const float* ssm, const float* chroma, const float* chroma_med,
                            const int64_t* block_off, const int32_t* n_blocks, int32_t n_tracks, int32_t max_blocks,
                            int32_t d_mfcc, int32_t d_ssm, int32_t d_chroma, const int32_t* pairs, int64_t n_pairs,
                            double kappa, int32_t K, float mu, int32_t binarize, double* scores_out, int32_t* seg_out,
                            int32_t path_cap, int32_t* len_out, int32_t* path_out, void* hip_stream);

/* acoss_earlyfusion_snf with `binarize` after mu and `binary_out` before the stream. binary_out:
 * NULL, or pair p's M x N binary matrix (uint8) as the Smith-Waterman kernel reads it, row-major at
 * binary_out[cross_off[p] ..); all zero for a pair that cannot be fused. cross_off is then required
 * (and checked against cross_total) even when cross_out is NULL. */
int acoss_earlyfusion_snf2(const float* mfcc, const float* ssm, const float* chroma, const float* chroma_med,
                           const int64_t* block_off, const int32_t* n_blocks, int32_t n_tracks, int32_t max_blocks,
                           int32_t d_mfcc, int32_t d_ssm, int32_t d_chroma, const int32_t* pairs, int64_t n_pairs,
                           double kappa, int32_t K, float mu, int32_t binarize, int32_t niters, double reg_diag,
                           double* score_out, const int64_t* cross_off, int64_t cross_total, double* cross_out,
                           uint8_t* binary_out, void* hip_stream);

/* The binarisation alone, for a batch of float32 matrices in acoss_sw_constrained's layout (matrix
 * b: rows[b] x cols[b], row-major at mats + off[b]; every array a device pointer): out (uint8, the
 * same offsets) = the row rule (ACOSS_EF_BIN_ROWS) or the mutual rule of each matrix. It runs the
 * pipeline's own kernels: the row launch acoss_earlyfusion would choose for ld = align_up(max(
 * max_rows, max_cols), 4) (so max_rows and max_cols pick the shape class), then the column pass,
 * on planes padded to ld x ld; a made-up bank (n_blocks = {rows0, cols0, rows1, cols1, ...}, pairs
 * (2 b, 2 b + 1)) stands for the tracks. ACOSS_E_ARG for kappa < 0, an unknown binarize, ld above
 * 16384, or a matrix with no rows or columns or more than max_rows x max_cols. */
int acoss_binarize_mutual(const float* mats, const int64_t* off, const int32_t* rows, const int32_t* cols,
                          int32_t n_mats, int32_t max_rows, int32_t max_cols, double kappa, int32_t binarize,
                          uint8_t* out, void* hip_stream);

/* EarlyFusion beat-synchronous block features of a batch of tracks (replaces
 * EarlyFusion.load_features' block loops, acoss/algorithms/earlyfusion_traile.py:67-154, and its
 * skimage resize_block, :214-247, restated in float64). Track t: chroma frames [frame_off[t],
 * +n_frames[t]) of chroma ((sum n) x 12) and MFCC frames [mfcc_off[t], +mfcc_frames[t]) of mfcc
 * ((sum n_mfcc) x d_mfcc, frame-major: mfcc_htk transposed, NaN already zeroed; the extractor's
 * mfcc_htk has fewer frames than the chroma, features.py:884); onsets (frame indices, int64) at
 * [onset_off[t], ...), its n_blocks = n_onsets - blocksize blocks at global block index
 * block_off[t] .. (total_blocks in all). Block b spans mfcc[o[b] : o[b+blocksize-1]] and
 * chroma[o[b] : o[b+blocksize]], each clamped to its own frame count as Python slicing does
 * (resize_block's X[i1:i2], :240); the caller guarantees every clamped span is non-empty (the
 * reference raises on an empty one). Outputs per global block: out_mfcc (mfccs_per_block *
 * d_mfcc), out_ssm (mfccs_per_block (mfccs_per_block - 1) / 2), out_chroma (chromas_per_block *
 * 12) float32; out_med (n_tracks x 12) = np.median(chroma, axis=0). */
int acoss_ef_block_features(const float* mfcc, const float* chroma, const int64_t* frame_off, const int32_t* n_frames,
                            const int64_t* mfcc_off, const int32_t* mfcc_frames,
                            const int64_t* onsets, const int64_t* onset_off, const int64_t* block_off,
                            int32_t n_tracks, int64_t total_blocks, int32_t blocksize, int32_t mfccs_per_block,
                            int32_t chromas_per_block, int32_t d_mfcc, float* out_mfcc, float* out_ssm,
                            float* out_chroma, float* out_med, void* hip_stream);

/* Finish of a pair-score matrix after the pair loop, in place when out == D.
 * D, out: (n x n) float32, row stride ld (elements). symmetric = 1 first forms D[i,j] + D[j,i] from
 * the original values (CoverAlgorithm.all_pairwise's `Ds += Ds.T`, algorithm_template.py:188-191);
 * mode 0 stops there, 1 divides by norm[j] (Serra09.normalize_by_length, rqa_serra09.py:71-83),
 * 2 stores norm[j] / D (ChenFusion.normalize_by_length, latefusion_chen.py:75-85); norm: float64[n]
 * = sqrt(frames of song j), the quotient taken in float64 and rounded to float32 as the
 * reference's float32 memmap does. */
int acoss_ds_finish(const float* D, int32_t n, int64_t ld, const double* norm, int32_t symmetric, int32_t mode,
                    float* out, void* hip_stream);

/* The rank step of CoverAlgorithm.getEvalStatistics (algorithm_template.py:206-291): for query q
 * (song q_song[q]) and each song j = members[m_off[q] .. m_off[q+1]), ranks_out[that index] = the
 * 1-based position of j in np.argsort(-D', 1, kind="stable") of the query's row, where D' is D
 * with the diagonal set to -inf (:234) and columns ordered by pos[] (each song's position in the
 * reference's clique ordering, :220-230; NaN scores sort last). D: (n x n) float32, stride ld. */
int acoss_eval_ranks(const float* D, int32_t n, int64_t ld, const int32_t* pos, const int32_t* q_song,
                     const int64_t* m_off, const int32_t* members, int32_t n_queries, int32_t* ranks_out,
                     void* hip_stream);

/* ---------------------------------------------------------------------------------
 * Per-track feature files (.npz twins of the reference's deepdish .h5 files), read on native
 * threads: replaces the per-song `dd.io.load` of CoverAlgorithm.load_features
 * (acoss/algorithms/algorithm_template.py:90) and EarlyFusion.load_features
 * (acoss/algorithms/earlyfusion_traile.py:88-99) for a whole batch of songs in two calls.
 * Host only (no GPU); every pointer is a HOST pointer. */
typedef struct acoss_npz_member {
  int32_t file;        /* index into paths */
  int32_t method;      /* zip method: 0 stored (np.savez), 8 deflate (np.savez_compressed) */
  int32_t ndim;
  int32_t fortran;     /* fortran_order of the .npy header */
  int64_t shape[8];
  int64_t nbytes;      /* bytes of array data (itemsize * prod(shape)) */
  int64_t member_off;  /* file offset of the member (the .npy stream) */
  int64_t comp_size;   /* its compressed size */
  int64_t npy_size;    /* its uncompressed size */
  int64_t data_skip;   /* offset of the array data inside the .npy stream */
  char name[128];      /* member name without ".npy", e.g. "madmom_features/onsets" */
  char descr[32];      /* numpy dtype descr, e.g. "<f4", "<U6" (object dtypes are refused) */
} acoss_npz_member;

/* Index n_files npz files: every member whose top-level key (the name up to the first '/') is
 * one of `keys_host` ('\n'-separated; NULL = every member), in file order, then zip order.
 * *n_out = the member count; ACOSS_E_ARG (message names the file) on an unreadable file or when
 * the count exceeds max_out (retry with *n_out). n_threads <= 0: every hardware thread. */
int acoss_npz_index(const char* const* paths_host, int32_t n_files, const char* keys_host, int32_t n_threads,
                    acoss_npz_member* out_host, int64_t max_out, int64_t* n_out);

/* Read every member's array data into dst_host[i] (nbytes each), one thread per file. */
int acoss_npz_read(const char* const* paths_host, const acoss_npz_member* members_host, int64_t n_members,
                   void* const* dst_host, int32_t n_threads);

#ifdef __cplusplus
}
#endif
#endif /* ACOSS_HIP_H */
