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

// The alignment DP (crp_dp.hip) over nb pairs' CRP words maskT (mstride words between pairs, row
// pitch ld, dims = (M', N') per pair, L = the longest M').
// launch_dp: align 0 = Qmax (serra09), 1 = dmax (chen17); eqg: go == ge; bnd: ceil(L / 2048) * ld
// records per pair (bstride between pairs); out[p] = the score.
void launch_dp(int align, bool eqg, int nb, int L, const uint32_t* maskT, int64_t mstride, int ld, const int2* dims,
               float go, float ge, float4* bnd, int64_t bstride, float* out, hipStream_t s);
// launch_trace: Qmax (qmax may be NULL) and seg[p] = (i0, j0, i1, j1), where its alignment starts
// and ends, for L <= kTraceMaxLen; bnd: trace_bnd_records(L, ld) records of kTraceRecBytes per pair.
constexpr int kTraceMaxLen = 65535;  // 16 bits per coordinate of a packed cell
constexpr size_t kTraceRecBytes = 32;
int64_t trace_bnd_records(int L, int ld);
void launch_trace(int nb, int L, const uint32_t* maskT, int64_t mstride, int ld, const int2* dims, float go, float ge,
                  void* bnd, int64_t bstride, float* qmax, int32_t* seg, hipStream_t s);
// The Qmax alignment path, cell by cell, for L <= kTraceMaxLen. launch_dir: the direction DP; per
// pair it fills a plane of 2-bit predecessor codes (dir_plane_bytes(L, ld) bytes, pstride bytes
// between pairs) and endkey[p] = (i1 << 16) | j1 (kNoEnd where Qmax is 0); qmax may be NULL; bnd:
// trace_bnd_records(L, ld) float4 records per pair. launch_backtrack: walks each pair's plane from
// its end cell and writes len[p] cells (i, j), first to last, to path + 2 path_cap p (the rest -1)
// and, unless seg is NULL, launch_trace's seg[p].
constexpr uint32_t kNoEnd = 0xffffffffu;
int64_t dir_plane_bytes(int L, int ld);
void launch_dir(int nb, int L, const uint32_t* maskT, int64_t mstride, int ld, const int2* dims, float go, float ge,
                float4* bnd, int64_t bstride, uint8_t* plane, int64_t pstride, uint32_t* endkey, float* qmax,
                hipStream_t s);
void launch_backtrack(int nb, const uint8_t* plane, int64_t pstride, int ld, const int2* dims, const uint32_t* endkey,
                      int path_cap, int32_t* seg, int32_t* len, int32_t* path, hipStream_t s);

}  // namespace acoss
