// crp_internal.hpp — what the Serra09/Chen translation units (crp.hip, crp_split.hip, crp_dp.hip)
// share.
#pragma once
#include "common.hpp"

namespace acoss {

// One batch of pairs of the Serra09/Chen path, all device pointers.
struct CrpBatch {
  const float* feats;    // packed (sum n, 12) chroma
  const float* feats2;   // per track (ldn frames): frames f, f+1 interleaved (24 floats); split path only
  const int64_t* off;    // track row offsets
  const int32_t* len;    // track frame counts
  const float* NX;       // stacked squared norms, track t at NX[t*ldn]
  int ldn;
  const int32_t* pairs;  // (P, 2) query, reference (already offset to the batch)
  const int32_t* oti;    // per pair OTI shift of the reference
  const int2* dims;      // per pair (M', N')
  int m, tau;
  const float* yrot;     // per pair: reference frames rolled by the pair's OTI (max_len x 12)
  int64_t yrot_stride;   // floats between consecutive pairs in yrot
};

// Constant-address-space view of read-only global data: wave-uniform loads through it
// become scalar (s_load) loads whose values live in SGPRs.
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(4))) const f32x4 cfloat4;

// Two-kernel CRP around one sweep (crp_split.hip): thresholds and mask words of nb pairs with
// m = 9, tau = 1 and lines of at most L <= 4096 codes; 1 = not covered (crp.hip's crp_masks
// decides by the same rule and runs the generic k_crp_select / k_crp_panel instead).
// kplanes: 2 planes of nb*kstride uint16 (16-bit key prefixes, row-major and strip-major).
int launch_crp_split(const CrpBatch& B, int nb, int L, float kappa, void* kplanes, int ldk,
                     int64_t kstride,
                     uint32_t* RT, float* thr_r, float* T_r, float* thr_c, float* T_c, int64_t thr_stride,
                     uint32_t* maskT, int64_t mask_stride, int ld, hipStream_t s);

// The OTI-binary CRP (crp_otib.hip k_crp_otib; the definition: include/acoss_hip.h, acoss_crp_params2):
// the mask words of nb pairs with stacked lengths of at most L, in the layout the DP consumes, the
// zero bits above M' in a pair's last strip included. B.oti holds the pairs' global OTI; B.yrot and
// B.feats2 are not read. Every m <= 64 and every tau. closer (one pair only, may be NULL): the
// (M' x N') uint8 counts of the transpositions strictly closer than the applied one.
int launch_otib(const CrpBatch& B, int nb, int L, int oti_rank, uint32_t* maskT, int64_t mask_stride, int ld,
                hipStream_t s, uint8_t* closer = nullptr);

// The alignment DP (crp_dp.hip) over nb pairs' CRP words maskT (mstride words between pairs, row
// pitch ld, dims = (M', N') per pair, L = the longest M').
// launch_dp: align 0 = Qmax (serra09), 1 = dmax (chen17); eqg: go == ge; bnd: ceil(L / 2048) * ld
// records per pair (bstride between pairs); out[p] = the score.
void launch_dp(int align, bool eqg, int nb, int L, const uint32_t* maskT, int64_t mstride, int ld, const int2* dims,
               float go, float ge, float4* bnd, int64_t bstride, float* out, hipStream_t s);
// launch_trace: the score (may be NULL) and seg[p] = (i0, j0, i1, j1), where its alignment starts and
// ends, for L <= kTraceMaxLen; align as launch_dp's (the definitions: include/acoss_hip.h,
// acoss_crp_locate and acoss_crp_locate_dmax); bnd: trace_bnd_records(L, ld) records of
// kTraceRecBytes per pair.
constexpr int kTraceMaxLen = 65535;  // 16 bits per coordinate of a packed cell
constexpr size_t kTraceRecBytes = 32;
int64_t trace_bnd_records(int L, int ld);
void launch_trace(int align, int nb, int L, const uint32_t* maskT, int64_t mstride, int ld, const int2* dims, float go,
                  float ge, void* bnd, int64_t bstride, float* score, int32_t* seg, hipStream_t s);
// The alignment path, cell by cell, for L <= kTraceMaxLen. launch_dir: the direction DP; per pair
// it fills a plane of 2-bit predecessor codes (dir_plane_bytes(L, ld) bytes, pstride bytes between
// pairs) and endkey[p] = (i1 << 16) | j1 (kNoEnd where the score is 0); score may be NULL; bnd:
// trace_bnd_records(L, ld) float4 records per pair. launch_backtrack: walks each pair's plane from
// its end cell (align 1 also reads the pair's CRP words) and writes len[p] cells (i, j), first to
// last, to path + 2 path_cap p (the rest -1) and, unless seg is NULL, launch_trace's seg[p].
constexpr uint32_t kNoEnd = 0xffffffffu;
int64_t dir_plane_bytes(int L, int ld);
void launch_dir(int align, int nb, int L, const uint32_t* maskT, int64_t mstride, int ld, const int2* dims, float go,
                float ge, float4* bnd, int64_t bstride, uint8_t* plane, int64_t pstride, uint32_t* endkey, float* score,
                hipStream_t s);
void launch_backtrack(int align, int nb, const uint8_t* plane, int64_t pstride, const uint32_t* maskT, int64_t mstride,
                      int ld, const int2* dims, const uint32_t* endkey, int path_cap, int32_t* seg, int32_t* len,
                      int32_t* path, hipStream_t s);

// Cross-recurrence quantification (k_crp_rqa; the definition: include/acoss_hip.h, acoss_crp_rqa):
// per pair the diagonal-line histogram of its CRP words, folded into counts[p] = (n_rec, n_lines,
// n_lines_min, n_pts_min), lmax[p], stats[p] = (RR, DET, LMEAN, ENTR) and hist[p][l] = H[l] for
// l < hist_cap; each of the four may be NULL. nbins: counters of the per-pair LDS histogram,
// nbins - 1 >= min(M', N') of every pair and <= kRqaMaxLine; bnd: rqa_bnd_records(L, ld) records of
// kRqaRecBytes per pair.
constexpr int kRqaMaxLine = 16383;  // the longest line the LDS histogram takes: 16,384 bins, 64 KiB
constexpr size_t kRqaRecBytes = 8;
int64_t rqa_bnd_records(int L, int ld);
void launch_rqa(int nb, int L, int nbins, const uint32_t* maskT, int64_t mstride, int ld, const int2* dims, int lmin,
                void* bnd, int64_t bstride, int64_t* counts, int32_t* lmax, double* stats, int hist_cap, int32_t* hist,
                hipStream_t s);

// The most cells a dmax (chen17) path of an M x N matrix can have: floor(2 (M + N) / 3) - 2 for
// M, N >= 3, none below. Proof. Call the cells with a DP value the chain X_0 .. X_n (X_n the end
// cell); all lie in rows and columns >= 2, so i + j is at least 4 at X_0 and at most M + N - 2 at
// X_n. From X_(t-1) to X_t the sum i + j grows by 2 on an a step, which adds one cell (X_t), and by
// 3 on a b or c step, which adds at most two (X_t and its intermediate). With s steps of the first
// and t of the second kind, 2 s + 3 t <= M + N - 6 =: F, and s + 2 t is largest at t = floor(F / 3),
// s = 1 if F mod 3 == 2 else 0, i.e. floor(2 F / 3) (a unit of i + j buys 1/2 cell by a, 2/3 by b or
// c). Before X_1 come X_0 and at most one more cell, the intermediate the path began on. Together
// 2 + floor(2 (M + N - 6) / 3) = floor(2 (M + N) / 3) - 2. The bound is met: 2 cells at 3 x 3, and
// the b / c staircases of tests/dmax_path_np.py come within two cells of it on square matrices. It
// grows with M and with N, so the bound at the longest stacked length serves every pair of a batch.
// The same number: acoss/_lib.py dmax_path_bound, tests/dmax_path_np.py path_bound.
__host__ __device__ constexpr int dmax_path_bound(int M, int N) {
  return (M < 3 || N < 3) ? 0 : 2 * (M + N) / 3 - 2;
}

}  // namespace acoss
