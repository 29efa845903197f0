// crp_dp.hip — the Qmax (serra09) / dmax (chen17) alignment DP over the CRP words that crp.hip
// and crp_split.hip produce: essentia CoverSongSimilarity('symmetric') restated, six kernels
// around one wavefront walk.
//
// A chain of lanes owns consecutive rows of the CRP (R rows each) and sweeps the columns skewed
// by one column per lane: lane l is at column c = s - l at step s, so the cells of one step lie
// on an anti-diagonal and every lane has its three predecessors ready. The last two rows of a
// lane pass down one lane per step with __shfl_up; where the CRP has more rows than a wave
// covers, bands of 64 R rows chain through a small HBM buffer. dp_walk is that walk, written
// once. What differs between the kernels is passed to it:
//  * a lane policy: what a lane keeps per column and the recurrence on it (step).
//      DpLane    f32 scores, any gamma and both alignments; FAST: serra09 at gamma = K/2
//      DpLanePk  chen17 at gamma = K/2 in packed 16-bit integers, two rows per instruction
//      DpLaneT   either alignment with the cell where each path began carried beside every score
//      DpLaneD   either alignment's scores that leave a 2-bit predecessor code per cell in a plane
//      DpLaneR   no alignment: the length of the diagonal run ending on each cell, counted where it ends
//  * an edge policy: what is above the chain's first lane and below its last one.
//      Band       the band above / below, through HBM records
//      GroupEdge  nothing above, nothing kept: several short pairs per wave, one band each
//  * the lane's index in its chain, the number of steps (wave-uniform) and the fetch of a
//    column's CRP word, which keeps each kernel's own bounds and masking.
//
//  k_crp_dp<ALIGN, EQG, R>   one wave per pair, DpLane in bands
//  k_crp_dp_fast<R>          the same with the FAST step
//  k_crp_dp_grp              FAST at 32 rows per lane, 64 / ceil(L / 32) pairs per wave
//  k_crp_dp_pk<1>            DpLanePk in bands
//  k_crp_dp_trace<ALIGN, EQG, R>  DpLaneT in bands, for acoss_crp_locate / acoss_locate_crp (ALIGN 0)
//                            and acoss_crp_locate_dmax / acoss_locate_crp_dmax (ALIGN 1)
//  k_crp_dp_dir<ALIGN, EQG, R>    DpLaneD in bands, and k_crp_backtrack / k_crp_backtrack_dmax, the walk
//                            back over its plane, for acoss_crp_path / acoss_path_crp and their _dmax twins
//  k_crp_rqa<R>              DpLaneR in bands and the fold of its line histogram, for acoss_crp_rqa /
//                            acoss_rqa_crp
// launch_dp, launch_trace, launch_dir and launch_rqa choose among them.
#include <cstdlib>
#include <type_traits>

#include "crp_internal.hpp"

namespace acoss {

// --------------------------------------------------------------------------------------
// The walk.
//   Lane:  Above (what goes down one lane per column; Above{} = nothing above), Col (one column
//          of the lane's rows), shfl_up(Above), step(new, col-1, col-2, w0, h0, c) -> Above, Np,
//          and the walk's history w1, w2, h1, h2 that step rotates.
//   Edge:  above(h, c, incol): h as shuffled, or what the edge supplies for the chain's first
//          lane; below(o, c, incol): keeps o where the chain's last lane has rows below it. Both
//          get the walk's one test of the column, incol = 0 <= c < Np, and hold whatever does not
//          change from step to step (which lane they act on, whether a band is there) ready-made.
//   fetch: CRP word of column c restricted to this lane's rows (0 outside the matrix).
// --------------------------------------------------------------------------------------
template <class Lane, class Edge, class Fetch>
__device__ __forceinline__ void dp_walk(Lane& L, const Edge& E, int idx, int S_end, Fetch fetch) {
  using Above = typename Lane::Above;
  using Col = typename Lane::Col;
  L.w1 = L.w2 = 0;
  L.h1 = L.h2 = Above{};
  // Three columns in rotation, so no column is ever copied: step s0 + k writes q[-k mod 3] from
  // q[1 - k mod 3] (column c-1) and q[2 - k mod 3] (column c-2). Separate arrays behind constant
  // indices: after the unroll each stays in registers of its own.
  Col qa{}, qb{}, qc{};
  Col* const q[3] = {&qa, &qb, &qc};
  Above pub{};  // what this lane hands down, one step late
  uint32_t wnext = fetch(-idx);
  for (int s0 = 0; s0 < S_end; s0 += 3) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int s = s0 + k;
      if (k > 0 && s >= S_end) break;
      const int c = s - idx;
      const uint32_t w0 = wnext;
      wnext = fetch(c + 1);  // the next column's word: its latency hides behind this step
      const bool incol = c >= 0 && c < L.Np;
      const Above h0 = E.above(Lane::shfl_up(pub), c, incol);
      pub = L.step(*q[(3 - k) % 3], *q[(4 - k) % 3], *q[(5 - k) % 3], w0, h0, c);
      E.below(pub, c, incol);
    }
  }
}

// bit r: 2 <= row0 + r < Mp (rows 0 and 1 of the matrix hold 0, like columns 0 and 1)
template <int R>
__device__ __forceinline__ uint32_t row_valid_mask(int row0, int Mp) {
  uint32_t rv = 0;
  for (int r = 0; r < R; ++r) rv |= (uint32_t)((row0 + r >= 2) && (row0 + r < Mp)) << r;
  return rv;
}

// Band `band` of pair p as lane `lane` sees it, at Lane::kRows rows per lane: where its rows and
// its CRP words are, and, as the walk's edge policy, the boundary records (bnd: one row of ld
// records per band and pair) that lane 0 reads from the band above and lane 63 writes for the
// band below.
template <class Lane>
struct Band {
  using Above = typename Lane::Above;
  using Rec = typename Lane::Rec;
  int row0, sh;          // this lane's first row, and its rows' place inside their 32-row strip word
  const uint32_t* mrow;  // that strip's words, one per column
  const Rec* bin;
  Rec* bout;
  bool first, reads, writes;  // lane 0; lane 0 with a band above; lane 63 with a band below

  __device__ __forceinline__ Band(int p, int band, int nbands, int lane, const uint32_t* maskT,
                                  int64_t mask_stride, int ld, Rec* bnd, int64_t bnd_stride)
      : row0((band * 64 + lane) * Lane::kRows), sh(row0 & 31),
        mrow(maskT + (size_t)p * mask_stride + (size_t)(row0 >> 5) * ld),
        bin(bnd + (size_t)p * bnd_stride + (size_t)(band - 1) * ld),
        bout(bnd + (size_t)p * bnd_stride + (size_t)band * ld),
        first(lane == 0), reads(lane == 0 && band > 0), writes(lane == 63 && band + 1 < nbands) {}
  __device__ __forceinline__ Above above(const Above& h, int c, bool incol) const {
    if (!first) return h;
    return (reads && incol) ? Lane::from_rec(bin[c]) : Above{};
  }
  __device__ __forceinline__ void below(const Above& o, int c, bool incol) const {
    if (writes && incol) bout[c] = Lane::to_rec(o);
  }
};

// A group of lanes that holds all rows of its pair: its first lane has nothing above.
template <class Lane>
struct GroupEdge {
  using Above = typename Lane::Above;
  bool first;  // the group's lane 0
  __device__ __forceinline__ Above above(const Above& h, int, bool) const { return first ? Above{} : h; }
  __device__ __forceinline__ void below(const Above&, int, bool) const {}
};

// --------------------------------------------------------------------------------------
// DpLane<ALIGN, EQG, R, FAST>: f32 scores. ALIGN 0 = serra09 (Qmax), 1 = chen17 (dmax); EQG:
// gamma_open == gamma_ext; R = 32, 16 or 8 rows per lane by the batch's longest CRP, so short
// tracks keep every lane busy.
// --------------------------------------------------------------------------------------
struct DpAbove {  // what lane l-1 (or the band above) hands down for one column
  float q30, q31;  // its last two rows (R-2, R-1)
  uint32_t b;      // bit0 = C[row R-2], bit1 = C[row R-1]
};

// FAST (serra09 with gamma_open == gamma_ext = K/2 >= 0, the reference's setting): every score is
// an exact multiple of 1/2, so "hit ? mx + 1 : max(mx - go, 0)" is max(fma(hit, 1 + go, mx - go), 0)
// exactly, and the validity masks move out of the row loop: the kernel zeroes the CRP words of
// columns < 2 and rows outside [2, Mp) at the fetch. Cells there then hold 0 (top-left: all their
// predecessors are 0) or at most max(0, best - go) (bottom/right: no hit, and they never feed a
// valid cell), so neither the valid scores nor their maximum change.
// v_cvt_f32_ubyteB: byte B of v as a float (the compiler emits only the byte-0 form plus shifts).
template <int B>
__device__ __forceinline__ float cvt_f32_ubyte(uint32_t v) {
  float f;
  if constexpr (B == 0) asm("v_cvt_f32_ubyte0 %0, %1" : "=v"(f) : "v"(v));
  else if constexpr (B == 1) asm("v_cvt_f32_ubyte1 %0, %1" : "=v"(f) : "v"(v));
  else if constexpr (B == 2) asm("v_cvt_f32_ubyte2 %0, %1" : "=v"(f) : "v"(v));
  else asm("v_cvt_f32_ubyte3 %0, %1" : "=v"(f) : "v"(v));
  return f;
}

// b is a constant after the row loops unroll, so the switch folds away
__device__ __forceinline__ float cvt_f32_ubyte_n(uint32_t v, int b) {
  switch (b) {
    case 0: return cvt_f32_ubyte<0>(v);
    case 1: return cvt_f32_ubyte<1>(v);
    case 2: return cvt_f32_ubyte<2>(v);
    default: return cvt_f32_ubyte<3>(v);
  }
}

template <int ALIGN, bool EQG, int R, bool FAST = false>
struct DpLane {
  static constexpr int kRows = R;
  using Above = DpAbove;
  using Rec = float4;  // q30, q31, bits as float, unused
  using Col = float[R];  // one column: this lane's R scores
  static __device__ __forceinline__ Above shfl_up(const Above& a) {
    return Above{__shfl_up(a.q30, 1), __shfl_up(a.q31, 1), (uint32_t)__shfl_up((int)a.b, 1)};
  }
  static __device__ __forceinline__ Above from_rec(const Rec& v) { return Above{v.x, v.y, (uint32_t)v.z}; }
  static __device__ __forceinline__ Rec to_rec(const Above& o) { return make_float4(o.q30, o.q31, (float)o.b, 0.0f); }

  float go, ge;
  int Np;
  uint32_t rowvalid;  // bit r: 2 <= global row < Mp
  uint32_t w1, w2;    // CRP words of columns c-1, c-2 (bit r = row r)
  DpAbove h1, h2;     // from above for columns c-1, c-2
  float best;

  __device__ __forceinline__ float gam(uint32_t bit) const { return EQG ? go : (bit ? go : ge); }

  // qn: new column c; q1: column c-1; q2: column c-2. w0: CRP word of column c;
  // h0: from above for column c. Returns the values to hand to the lane below.
  __device__ __forceinline__ DpAbove step(Col& qn, const Col& q1, const Col& q2, uint32_t w0, const DpAbove& h0,
                                          int c) {
    const bool colvalid = (c >= 2) && (c < Np);
    const uint32_t vmask = colvalid ? rowvalid : 0u;
    // extended words: bit r+2 <-> row r; bits 0,1 <-> rows -2,-1 (from above)
    const uint64_t e0 = ((uint64_t)w0 << 2) | h0.b;
    const uint64_t e1 = ((uint64_t)w1 << 2) | h1.b;
    const uint64_t e2 = ((uint64_t)w2 << 2) | h2.b;
    if constexpr (FAST) {
      // two rows per v_pk_add_f32 / v_pk_fma_f32; the hit bits as bytes (rows k, k+8, k+16, k+24
      // of one masked word), one v_cvt_f32_ubyteN each
      typedef float dp_f32x2 __attribute__((ext_vector_type(2)));
      const dp_f32x2 g1 = {1.0f + go, 1.0f + go};
      const dp_f32x2 ngo = {-go, -go};
      uint32_t bm[R < 8 ? R : 8];
#pragma unroll
      for (int k = 0; k < (R < 8 ? R : 8); ++k) bm[k] = (w0 >> k) & 0x01010101u;
#pragma unroll
      for (int r = 0; r < R; r += 2) {
        float mxs[2], hb[2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          const int rr = r + e;
          const float Qa = rr >= 1 ? q1[rr - 1] : h1.q31;
          const float Qb = rr >= 2 ? q1[rr - 2] : (rr == 1 ? h1.q31 : h1.q30);
          const float Qc = rr >= 1 ? q2[rr - 1] : h2.q31;
          mxs[e] = fmaxf(fmaxf(Qa, Qb), Qc);
          hb[e] = cvt_f32_ubyte_n(bm[rr & 7], rr >> 3);
        }
        const dp_f32x2 mx = {mxs[0], mxs[1]};
        const dp_f32x2 hv = {hb[0], hb[1]};
        const dp_f32x2 t = __builtin_elementwise_fma(hv, g1, mx + ngo);
        asm("v_max3_f32 %0, %1, %2, %3" : "=v"(best) : "v"(best), "v"(t.x), "v"(t.y));
        qn[r] = fmaxf(t.x, 0.0f);
        qn[r + 1] = fmaxf(t.y, 0.0f);
      }
    } else {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const float Qa = r >= 1 ? q1[r - 1] : h1.q31;                            // Q[r-1][c-1]
      float Qb = r >= 2 ? q1[r - 2] : (r == 1 ? h1.q31 : h1.q30);              // Q[r-2][c-1]
      float Qc = r >= 1 ? q2[r - 1] : h2.q31;                                  // Q[r-1][c-2]
      if (ALIGN == 1) {
        Qb = Qb + (float)((e0 >> (r + 1)) & 1u);  // + C[r-1][c]
        Qc = Qc + (float)((e1 >> (r + 2)) & 1u);  // + C[r][c-1]
      }
      const bool hit = (e0 >> (r + 2)) & 1u;
      float v;
      if (EQG) {
        const float mx = fmaxf(fmaxf(Qa, Qb), Qc);
        v = hit ? mx + 1.0f : fmaxf(mx - go, 0.0f);
      } else {
        const float x = Qa - gam((e1 >> (r + 1)) & 1u);  // gamma(C[r-1][c-1])
        const float y = Qb - gam((e1 >> r) & 1u);        // gamma(C[r-2][c-1])
        const float z = Qc - gam((e2 >> (r + 1)) & 1u);  // gamma(C[r-1][c-2])
        const float miss = fmaxf(fmaxf(0.0f, x), fmaxf(y, z));
        v = hit ? fmaxf(fmaxf(Qa, Qb), Qc) + 1.0f : miss;
      }
      v = ((vmask >> r) & 1u) ? v : 0.0f;
      best = fmaxf(best, v);
      qn[r] = v;
    }
    }
    DpAbove out;
    out.q30 = qn[R - 2];
    out.q31 = qn[R - 1];
    out.b = (w0 >> (R - 2)) & 3u;
    h2 = h1;
    h1 = h0;
    w2 = w1;
    w1 = w0;
    return out;
  }
};

template <int ALIGN, bool EQG, int R, bool FAST>
__device__ __forceinline__ void crp_dp_body(const uint32_t* __restrict__ maskT, int64_t mask_stride, int ld,
                                               const int2* __restrict__ dims, float go, float ge,
                                               float4* __restrict__ bnd, int64_t bnd_stride,
                                               float* __restrict__ out) {
  using Lane = DpLane<ALIGN, EQG, R, FAST>;
  const int p = blockIdx.x;
  const int lane = threadIdx.x;
  const int2 dm = dims[p];
  const int Mp = dm.x, Np = dm.y;
  const int nbands = (Mp + 64 * R - 1) / (64 * R);
  Lane L;
  L.go = go;
  L.ge = ge;
  L.Np = Np;
  L.best = 0.0f;
  for (int band = 0; band < nbands; ++band) {
    const Band<Lane> B(p, band, nbands, lane, maskT, mask_stride, ld, bnd, bnd_stride);
    const uint32_t rv = L.rowvalid = row_valid_mask<R>(B.row0, Mp);
    const bool lane_active = B.row0 < Mp;
    dp_walk(L, B, lane, Np + 63, [&](int c) -> uint32_t {
      if (!(lane_active && c >= (FAST ? 2 : 0) && c < Np)) return 0u;
      const uint32_t w = B.mrow[c];
      const uint32_t wr = R == 32 ? w : (w >> B.sh) & ((1u << (R & 31)) - 1u);
      return FAST ? (wr & rv) : wr;
    });
    __threadfence_block();
    __syncthreads();
  }
  const float best = wave_max(L.best);
  if (lane == 0) out[p] = best;
}

template <int ALIGN, bool EQG, int R>
__global__ __launch_bounds__(64) void k_crp_dp(const uint32_t* __restrict__ maskT, int64_t mask_stride, int ld,
                                               const int2* __restrict__ dims, float go, float ge,
                                               float4* __restrict__ bnd, int64_t bnd_stride,
                                               float* __restrict__ out) {
  crp_dp_body<ALIGN, EQG, R, false>(maskT, mask_stride, ld, dims, go, ge, bnd, bnd_stride, out);
}

// No occupancy hint: left alone the FAST body takes what it wants at R = 32 (160 VGPRs, 3 waves per
// SIMD, today), which measured faster than forcing it into 128 (4 waves per SIMD): 14.2 vs 14.8 ms
// per covers80 step.
template <int R>
__global__ __launch_bounds__(64) void k_crp_dp_fast(
    const uint32_t* __restrict__ maskT, int64_t mask_stride, int ld, const int2* __restrict__ dims, float go, float ge,
    float4* __restrict__ bnd, int64_t bnd_stride, float* __restrict__ out) {
  crp_dp_body<0, true, R, true>(maskT, mask_stride, ld, dims, go, ge, bnd, bnd_stride, out);
}

// --------------------------------------------------------------------------------------
// k_crp_dp_grp: the FAST DP (serra09, gamma_open == gamma_ext = K/2) with SEVERAL pairs per
// wave for CRPs of at most 2048 rows: a group of LP = ceil(L / 32) lanes per pair (lane ll owns
// rows 32 ll .. 32 ll + 31, one band), G = 64 / LP groups per wave. A one-pair wave walks
// N' + 63 steps however short the pair; a group walks N' + LP - 1, and every lane keeps 32 rows
// per step, so short tracks (Da-TACOS lengths: L ~ 500) no longer leave most lanes idle or pay
// the per-step shuffles for 8 rows. Same recurrence, same DpLane step: bit-identical scores.
// --------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_crp_dp_grp(const uint32_t* __restrict__ maskT, int64_t mask_stride, int ld,
                                                   const int2* __restrict__ dims, int nb, int LP, float go,
                                                   float* __restrict__ out) {
  constexpr int R = 32;
  using Lane = DpLane<0, true, R, true>;
  __shared__ float s_best[64];
  const int lane = threadIdx.x;
  const int G = 64 / LP;
  const int g = lane / LP, ll = lane - g * LP;
  const int p = blockIdx.x * G + g;
  const bool in_group = g < G && p < nb;
  const int2 dm = in_group ? dims[p] : make_int2(0, 0);
  const int Mp = dm.x, Np = dm.y;
  const int row0 = ll * R;
  const uint32_t* mrow = maskT + (size_t)(in_group ? p : 0) * mask_stride + (size_t)ll * ld;
  Lane L;
  L.go = go;
  L.ge = go;
  L.Np = Np;
  L.best = 0.0f;
  const uint32_t rv = L.rowvalid = row_valid_mask<R>(row0, Mp);
  // steps until every group of the wave is done (wave-uniform bound)
  const int S_end = (int)wave_max_u32(in_group ? (unsigned)(Np + LP - 1) : 0u);
  const bool lane_active = in_group && row0 < Mp;
  dp_walk(L, GroupEdge<Lane>{ll == 0}, ll, S_end, [&](int c) -> uint32_t {
    if (!(lane_active && c >= 2 && c < Np)) return 0u;
    return mrow[c] & rv;
  });
  // per-group maximum through LDS (groups need not be a power of two wide)
  s_best[lane] = L.best;
  __syncthreads();
  if (in_group && ll == 0) {
    float b = 0.0f;
    for (int k = 0; k < LP; ++k) b = fmaxf(b, s_best[lane + k]);
    out[p] = b;
  }
}

// --------------------------------------------------------------------------------------
// k_crp_dp_pk<ALIGN>: k_crp_dp<ALIGN, true, 32> in packed 16-bit integers. With
// gamma_open == gamma_ext = K/2 (K a small integer, 1 for the reference's 0.5), every score is
// a multiple of 1/2, so 2Q is an exact integer below 4 L: lane l keeps rows (h, h + 16) of a
// column in one u32 (row h low, row h + 16 high) and takes two rows per v_pk_max_u16 /
// v_pk_add_u16 / saturating v_pk_sub_u16 (max(x - K, 0) in one instruction). The predecessor
// rows of pair h are pair h - 1 / h - 2 of the previous columns; pairs 0 and 1 splice in the
// rows handed down by the lane above (v_perm). Bit-identical to the f32 kernel: both compute
// the same exact multiples of 1/2 (the f32 values never round). Only ALIGN = 1 is launched:
// serra09 at these gammas has the FAST step.
// --------------------------------------------------------------------------------------
typedef unsigned short dp_u16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned pk16(dp_u16x2 v) { return __builtin_bit_cast(unsigned, v); }
__device__ __forceinline__ dp_u16x2 up16(unsigned v) { return __builtin_bit_cast(dp_u16x2, v); }
__device__ __forceinline__ unsigned pk_max16(unsigned a, unsigned b) { return pk16(__builtin_elementwise_max(up16(a), up16(b))); }
__device__ __forceinline__ unsigned pk_add16(unsigned a, unsigned b) { return pk16(up16(a) + up16(b)); }
__device__ __forceinline__ unsigned pk_sub16(unsigned a, unsigned b) { return pk16(up16(a) - up16(b)); }
__device__ __forceinline__ unsigned pk_subsat16(unsigned a, unsigned b) {
  return pk16(__builtin_elementwise_sub_sat(up16(a), up16(b)));
}

struct DpAbovePk {  // what lane l-1 (or the band above) hands down for one column
  unsigned hq;      // its rows 30 (low half) and 31 (high half), x2 units
  uint32_t b;       // bit0 = C[row 30], bit1 = C[row 31]
};

template <int ALIGN>
struct DpLanePk {
  static constexpr int kRows = 32;
  using Above = DpAbovePk;
  using Rec = float4;  // hq and b as bit patterns, two unused
  using Col = unsigned[16];  // one column: rows (h, h + 16) in word h
  static __device__ __forceinline__ Above shfl_up(const Above& a) {
    return Above{(unsigned)__shfl_up((int)a.hq, 1), (uint32_t)__shfl_up((int)a.b, 1)};
  }
  static __device__ __forceinline__ Above from_rec(const Rec& v) {
    return Above{__builtin_bit_cast(unsigned, v.x), __builtin_bit_cast(unsigned, v.y)};
  }
  static __device__ __forceinline__ Rec to_rec(const Above& o) {
    return make_float4(__builtin_bit_cast(float, o.hq), __builtin_bit_cast(float, o.b), 0.0f, 0.0f);
  }

  unsigned K;          // gamma in x2 units, both halves
  int Np;
  uint32_t rz0, rz1;   // AND masks of pairs 0 / 1: rows 0 and 1 of the first band are 0
  uint32_t w1, w2;     // CRP words of columns c-1, c-2
  DpAbovePk h1, h2;    // from above for columns c-1, c-2
  unsigned best;

  __device__ __forceinline__ DpAbovePk step(Col& pn, const Col& p1, const Col& p2, uint32_t w0, const DpAbovePk& h0,
                                            int c) {
    const bool colok = (c >= 2) && (c < Np);
    // rows (-1, 15) and (-2, 14) of column c-1, (-1, 15) of column c-2
    const unsigned a0 = __builtin_amdgcn_perm(p1[15], h1.hq, 0x05040302u);
    const unsigned b0 = __builtin_amdgcn_perm(p1[14], h1.hq, 0x05040100u);
    const unsigned c0 = __builtin_amdgcn_perm(p2[15], h2.hq, 0x05040302u);
#pragma unroll
    for (int h = 0; h < 16; ++h) {
      const unsigned A = h >= 1 ? p1[h - 1] : a0;                  // Q[r-1][c-1]
      unsigned B = h >= 2 ? p1[h - 2] : (h == 1 ? a0 : b0);        // Q[r-2][c-1]
      unsigned Cq = h >= 1 ? p2[h - 1] : c0;                       // Q[r-1][c-2]
      if (ALIGN == 1) {
        const unsigned cb = h >= 1 ? (w0 >> (h - 1)) & 0x10001u : ((h0.b >> 1) & 1u) | (((w0 >> 15) & 1u) << 16);
        B = pk_add16(B, cb << 1);                                  // + C[r-1][c]
        Cq = pk_add16(Cq, ((w1 >> h) & 0x10001u) << 1);            // + C[r][c-1]
      }
      const unsigned mx = pk_max16(pk_max16(A, B), Cq);
      const unsigned m = pk_sub16(0u, (w0 >> h) & 0x10001u);      // 0xffff where C[r][c] = 1
      unsigned v = (m & pk_add16(mx, 0x00020002u)) | (~m & pk_subsat16(mx, K));
      if (h == 0) v &= rz0;
      if (h == 1) v &= rz1;
      v = colok ? v : 0u;
      best = pk_max16(best, v);
      pn[h] = v;
    }
    DpAbovePk out;
    out.hq = __builtin_amdgcn_perm(pn[15], pn[14], 0x07060302u);
    out.b = (w0 >> 30) & 3u;
    h2 = h1;
    h1 = h0;
    w2 = w1;
    w1 = w0;
    return out;
  }
};

// 4 waves per SIMD, no more: the body fits 96 registers (5 waves), and a launch of 4,000 pairs then
// measured 5.0 ms against 4.2 ms at 4 waves.
template <int ALIGN>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4, 4))) void k_crp_dp_pk(
    const uint32_t* __restrict__ maskT, int64_t mask_stride, int ld, const int2* __restrict__ dims, unsigned K,
    float4* __restrict__ bnd, int64_t bnd_stride, float* __restrict__ out) {
  using Lane = DpLanePk<ALIGN>;
  const int p = blockIdx.x;
  const int lane = threadIdx.x;
  const int2 dm = dims[p];
  const int Mp = dm.x, Np = dm.y;
  const int nbands = (Mp + 2047) / 2048;
  Lane L;
  L.K = K * 0x10001u;
  L.Np = Np;
  L.best = 0u;
  for (int band = 0; band < nbands; ++band) {
    const Band<Lane> B(p, band, nbands, lane, maskT, mask_stride, ld, bnd, bnd_stride);
    L.rz0 = L.rz1 = B.row0 == 0 ? 0xffff0000u : 0xffffffffu;
    const bool lane_active = B.row0 < Mp;
    dp_walk(L, B, lane, Np + 63,
            [&](int c) -> uint32_t { return (lane_active && c >= 0 && c < Np) ? B.mrow[c] : 0u; });
    __threadfence_block();
    __syncthreads();
  }
  const unsigned b2 = max(L.best & 0xffffu, L.best >> 16);
  const float r = wave_max(0.5f * (float)b2);
  if (lane == 0) out[p] = r;
}

// --------------------------------------------------------------------------------------
// k_crp_dp_trace<EQG, R>: the serra09 DP of k_crp_dp<0, ., R> with ORIGIN PROPAGATION: every
// cell carries, beside its score, the packed cell (i0 << 16) | j0 where its path began, and the
// wave reduces (Qmax, end cell, origin of the end cell) instead of a bare maximum. Memory per
// pair stays O(1) beyond the DP's own: no M' x N' score matrix is written.
//  * predecessors in the fixed order a = (i-1, j-1), b = (i-2, j-1), c = (i-1, j-2); the origin is
//    that of the FIRST predecessor attaining the maximum (raw values on a hit, penalised values
//    on a miss; a strictly greater value replaces, an equal one does not); a hit whose
//    predecessors are all 0 starts a path at itself.
//  * the end cell is the first cell in row-major order holding Qmax. The skewed walk does not
//    visit cells in row-major order, so every update compares the packed end key (i << 16) | j:
//    v > best || (v == best && v > 0 && key < bestkey). Inside one step a lane's cells share a
//    column and come in ascending rows, so there "first wins" is the strict compare alone.
//  * general arithmetic, validity per cell (any gamma). EQG = true is launched only where
//    gamma_open == gamma_ext = K/2 (K a small non-negative integer): every score is then an exact
//    multiple of 1/2, x - gamma never rounds, and the first maximum of the penalised values is the
//    first maximum of the raw ones, so one select serves hit and miss. Origins are defined where
//    a path can only begin on a hit, i.e. for gamma >= 0.
//  * R = 8 rows per lane for CRPs of at most 512 rows, R = 16 above (bands of 64 R rows): three
//    rotating columns of R scores and R origins are 6 R live registers. A launch takes the pairs
//    with row_lo < M' <= row_hi and leaves the others to the launch of the other R.
//  * the values handed to the next lane, and across a band boundary through HBM, are the last two
//    rows' scores, CRP bits and origins (TraceRec).
//  * ALIGN = 1 is chen17 (dmax; the definition: include/acoss_hip.h, acoss_crp_locate_dmax): b and
//    c carry the bonus bits C[r-1][c] and C[r][c-1], taken from the extended words as DpLane<1>
//    takes them (row 0 of a lane reads the last row of the lane or band above), and where such a
//    predecessor scores 0 its origin is the intermediate cell's key, key - 65536 for b and key - 1
//    for c: if that choice wins with a positive value, the intermediate is a hit and the path
//    begins there. The bonus is added before the common subtraction, so the halves select holds.
//    Two more selects per cell: 106 registers at R = 8 (4 waves per SIMD), 168 at R = 16 (3).
// Every lane runs every step and selects; the only branches around a shuffle are wave-uniform.
// --------------------------------------------------------------------------------------
struct DpAboveT {   // what lane l-1 (or the band above) hands down for one column
  float q30, q31;   // scores of its last two rows (R-2, R-1)
  uint32_t b;       // bit0 = C[row R-2], bit1 = C[row R-1]
  uint32_t o30, o31;  // origins of the same two cells
};

struct TraceRec {  // one column of a band boundary, 32 B
  float4 q;        // q30, q31, bits as float, unused
  uint4 o;         // o30, o31, unused
};
static_assert(sizeof(TraceRec) == kTraceRecBytes, "callers size the boundary buffer by kTraceRecBytes");

template <int ALIGN, bool EQG, int R>
struct DpLaneT {
  static_assert(R <= 16, "the extended CRP words are 32-bit");
  static constexpr int kRows = R;
  using Above = DpAboveT;
  using Rec = TraceRec;
  struct Col {  // scores and origins of one column
    float q[R];
    uint32_t o[R];
  };
  static __device__ __forceinline__ Above shfl_up(const Above& a) {
    return Above{__shfl_up(a.q30, 1), __shfl_up(a.q31, 1), (uint32_t)__shfl_up((int)a.b, 1),
                 (uint32_t)__shfl_up((int)a.o30, 1), (uint32_t)__shfl_up((int)a.o31, 1)};
  }
  static __device__ __forceinline__ Above from_rec(const Rec& v) {
    return Above{v.q.x, v.q.y, (uint32_t)v.q.z, v.o.x, v.o.y};
  }
  static __device__ __forceinline__ Rec to_rec(const Above& a) {
    return Rec{make_float4(a.q30, a.q31, (float)a.b, 0.0f), make_uint4(a.o30, a.o31, 0u, 0u)};
  }

  float go, ge;
  int Np;
  uint32_t rowvalid;  // bit r: 2 <= global row < Mp
  uint32_t key0;      // (global row of this lane's row 0) << 16
  uint32_t w1, w2;    // CRP words of columns c-1, c-2 (bit r = row r)
  DpAboveT h1, h2;    // from above for columns c-1, c-2
  float best;         // this lane's maximum so far, its end key and the origin of that cell
  uint32_t bkey, borg;

  // cn: new column c; c1: column c-1; c2: column c-2.
  __device__ __forceinline__ DpAboveT step(Col& cn, const Col& c1, const Col& c2, uint32_t w0, const DpAboveT& h0,
                                           int c) {
    const bool colvalid = (c >= 2) && (c < Np);
    const uint32_t vmask = colvalid ? rowvalid : 0u;
    // extended words: bit r+2 <-> row r; bits 0,1 <-> rows -2,-1 (from above)
    const uint32_t e0 = (w0 << 2) | h0.b;
    const uint32_t e1 = (w1 << 2) | h1.b;
    const uint32_t e2 = (w2 << 2) | h2.b;
    const uint32_t kc = key0 + (uint32_t)c;  // key of (row 0, c); only used where colvalid
    const float g_open = go, g_ext = ge;     // by value: a select between members is a select of addresses
    auto gam = [&](uint32_t bit) { return bit ? g_open : g_ext; };
    float cb = 0.0f;                         // this column's first maximum, its key and origin
    uint32_t ck = 0u, co = 0u;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const float Qa = r >= 1 ? c1.q[r - 1] : h1.q31;                        // Q[r-1][c-1]
      float Qb = r >= 2 ? c1.q[r - 2] : (r == 1 ? h1.q31 : h1.q30);          // Q[r-2][c-1]
      float Qc = r >= 1 ? c2.q[r - 1] : h2.q31;                              // Q[r-1][c-2]
      const uint32_t Oa = r >= 1 ? c1.o[r - 1] : h1.o31;
      uint32_t Ob = r >= 2 ? c1.o[r - 2] : (r == 1 ? h1.o31 : h1.o30);
      uint32_t Oc = r >= 1 ? c2.o[r - 1] : h2.o31;
      if constexpr (ALIGN == 1) {
        // chen17: a path that comes through b or c from a cell that scores 0 begins on the
        // intermediate cell the bonus paid for, (i-1, j) or (i, j-1); then the bonus itself
        const uint32_t xkey = kc + ((uint32_t)r << 16);
        Ob = Qb > 0.0f ? Ob : xkey - 65536u;
        Oc = Qc > 0.0f ? Oc : xkey - 1u;
        Qb = Qb + (float)((e0 >> (r + 1)) & 1u);  // + C[r-1][c]
        Qc = Qc + (float)((e1 >> (r + 2)) & 1u);  // + C[r][c-1]
      }
      const bool hit = (e0 >> (r + 2)) & 1u;
      float pa = Qa, pb = Qb, pc = Qc;
      if (!EQG) {
        const float x = Qa - gam((e1 >> (r + 1)) & 1u);  // gamma(C[r-1][c-1])
        const float y = Qb - gam((e1 >> r) & 1u);        // gamma(C[r-2][c-1])
        const float z = Qc - gam((e2 >> (r + 1)) & 1u);  // gamma(C[r-1][c-2])
        pa = hit ? Qa : x;
        pb = hit ? Qb : y;
        pc = hit ? Qc : z;
      }
      float mx = pa;
      uint32_t o = Oa;
      if (pb > mx) {
        mx = pb;
        o = Ob;
      }
      if (pc > mx) {
        mx = pc;
        o = Oc;
      }
      float v = hit ? mx + 1.0f : fmaxf(EQG ? mx - g_open : mx, 0.0f);
      const uint32_t key = kc + ((uint32_t)r << 16);
      o = (hit && !(mx > 0.0f)) ? key : o;  // all predecessors 0: the path starts here
      v = ((vmask >> r) & 1u) ? v : 0.0f;
      if (v > cb) {
        cb = v;
        ck = key;
        co = o;
      }
      // Pin the origin next to its score: the origins are first read in a later basic block
      // (the next step's shuffles), so the compiler sinks their selects there and carries every
      // compare mask (4 per cell, a scalar register pair each) across: 279 scalar spills at R = 16.
      asm volatile("" : "+v"(o));
      cn.q[r] = v;
      cn.o[r] = o;
    }
    if (cb > best || (cb == best && cb > 0.0f && ck < bkey)) {
      best = cb;
      bkey = ck;
      borg = co;
    }
    DpAboveT out;
    out.q30 = cn.q[R - 2];
    out.q31 = cn.q[R - 1];
    out.b = (w0 >> (R - 2)) & 3u;
    out.o30 = cn.o[R - 2];
    out.o31 = cn.o[R - 1];
    h2 = h1;
    h1 = h0;
    w2 = w1;
    w1 = w0;
    return out;
  }
};

// bnd: ceil(L / (64 R)) * ld TraceRec per pair (bnd_stride records between pairs); only read and
// written by CRPs of more than one band. qmax_out may be NULL; seg_out: int32[4] (i0, j0, i1, j1) per pair.
// Waves per SIMD: R = 8 needs 96 registers, exactly the step of 5 waves, and without the floor the
// unequal-gamma body lands at 100 (4 waves); R = 16 runs at 2 waves or better. chen17 at R = 8 needs
// 106 (126 with unequal gammas): 4 waves.
constexpr int trace_waves(int align, int R) { return R == 8 ? (align == 0 ? 5 : 4) : 2; }

template <int ALIGN, bool EQG, int R>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(trace_waves(ALIGN, R)))) void k_crp_dp_trace(
    const uint32_t* __restrict__ maskT, int64_t mask_stride, int ld, const int2* __restrict__ dims, int row_lo,
    int row_hi, float go, float ge, TraceRec* __restrict__ bnd, int64_t bnd_stride, float* __restrict__ qmax_out,
    int32_t* __restrict__ seg_out) {
  using Lane = DpLaneT<ALIGN, EQG, R>;
  const int p = blockIdx.x;
  const int lane = threadIdx.x;
  const int2 dm = dims[p];
  const int Mp = dm.x, Np = dm.y;
  if (!(Mp > row_lo && Mp <= row_hi)) return;  // the other R's launch takes this pair (wave-uniform)
  const int nbands = (Mp + 64 * R - 1) / (64 * R);
  Lane L;
  L.go = go;
  L.ge = ge;
  L.Np = Np;
  L.best = 0.0f;
  L.bkey = L.borg = 0u;
  for (int band = 0; band < nbands; ++band) {
    const Band<Lane> B(p, band, nbands, lane, maskT, mask_stride, ld, bnd, bnd_stride);
    L.rowvalid = row_valid_mask<R>(B.row0, Mp);
    L.key0 = (uint32_t)B.row0 << 16;
    const bool lane_active = B.row0 < Mp;
    dp_walk(L, B, lane, Np + 63, [&](int c) -> uint32_t {
      if (!(lane_active && c >= 0 && c < Np)) return 0u;
      return (B.mrow[c] >> B.sh) & ((1u << R) - 1u);
    });
    __threadfence_block();
    __syncthreads();
  }
  // wave reduction of (best, end key, origin) by the same rule as the per-cell update
  float best = L.best;
  uint32_t bkey = L.bkey, borg = L.borg;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float v = __shfl_xor(best, o);
    const uint32_t k = (uint32_t)__shfl_xor((int)bkey, o);
    const uint32_t g = (uint32_t)__shfl_xor((int)borg, o);
    if (v > best || (v == best && v > 0.0f && k < bkey)) {
      best = v;
      bkey = k;
      borg = g;
    }
  }
  if (lane == 0) {
    if (qmax_out) qmax_out[p] = best;
    const bool any = best > 0.0f;
    int32_t* sg = seg_out + 4 * (size_t)p;
    sg[0] = any ? (int)(borg >> 16) : -1;
    sg[1] = any ? (int)(borg & 0xffffu) : -1;
    sg[2] = any ? (int)(bkey >> 16) : -1;
    sg[3] = any ? (int)(bkey & 0xffffu) : -1;
  }
}

// --------------------------------------------------------------------------------------
// k_crp_dp_dir<EQG, R>: the serra09 DP of k_crp_dp_trace with, instead of an origin beside every
// score, a 2-BIT DIRECTION per cell written to a per-pair plane, so that k_crp_backtrack can
// follow the Qmax alignment cell by cell (acoss_crp_path / acoss_path_crp).
//  * scores only: the lane, its columns and what it hands down are DpLane's (DpAbove, float4
//    band records); same arithmetic and same choice of predecessor as DpLaneT, EQG included.
//  * code of a cell: 0 = no predecessor (its score is 0, or it is a hit whose predecessors are
//    all 0: a path starts there), 1 / 2 / 3 = a / b / c, the first one attaining the maximum.
//    Cells outside validity have score 0 and so code 0.
//  * the codes of a lane's R rows in one column are one word of 2 R bits (row r in bits 2r,
//    2r + 1), stored once per step with a plain vector store. Plane of a pair: row groups of R
//    rows, ld words each: word (i / R) * ld + j holds cell (i, j); 16-bit words at R = 8, 32-bit
//    at R = 16, both M' N' / 4 bytes. A lane that owns rows of the matrix stores every column, so
//    every word a walk can reach is written and the plane is never zeroed.
//  * R and the bands are the tracing DP's: R = 8 up to 512 rows, 16 above, by the same two
//    launches; the wave reduces (Qmax, end key) by its rule and leaves the key in endkey[p].
//  * ALIGN = 1 is chen17: the same codes over the values with their bonus; what else the walk
//    back needs (is the intermediate cell a hit, does the predecessor score above 0) it reads off
//    the CRP words and the plane itself, see k_crp_backtrack_dmax.
// The store sits after the step's shuffles, under the lane's own predicate; every lane runs every
// step.
// --------------------------------------------------------------------------------------
constexpr int kTraceShortRows = 512;  // R = 8 up to here, R = 16 above (tracing and direction DP)

template <int R>
struct DirWord {
  using type = uint32_t;
};
template <>
struct DirWord<8> {
  using type = uint16_t;
};

template <int ALIGN, bool EQG, int R>
struct DpLaneD {
  static_assert(R == 8 || R == 16, "2 R code bits are one 16- or 32-bit word");
  static constexpr int kRows = R;
  using Above = DpAbove;
  using Rec = float4;  // q30, q31, bits as float, unused
  using Col = float[R];
  using Word = typename DirWord<R>::type;
  static __device__ __forceinline__ Above shfl_up(const Above& a) {
    return Above{__shfl_up(a.q30, 1), __shfl_up(a.q31, 1), (uint32_t)__shfl_up((int)a.b, 1)};
  }
  static __device__ __forceinline__ Above from_rec(const Rec& v) { return Above{v.x, v.y, (uint32_t)v.z}; }
  static __device__ __forceinline__ Rec to_rec(const Above& o) { return make_float4(o.q30, o.q31, (float)o.b, 0.0f); }

  float go, ge;
  int Np;
  uint32_t rowvalid;  // bit r: 2 <= global row < Mp
  uint32_t key0;      // (global row of this lane's row 0) << 16
  uint32_t w1, w2;    // CRP words of columns c-1, c-2 (bit r = row r)
  DpAbove h1, h2;     // from above for columns c-1, c-2
  float best;         // this lane's maximum so far and its end key
  uint32_t bkey;
  Word* drow;         // this lane's row group of the direction plane, one word per column
  bool stores;        // the lane owns rows of the matrix

  __device__ __forceinline__ DpAbove step(Col& qn, const Col& q1, const Col& q2, uint32_t w0, const DpAbove& h0,
                                          int c) {
    const bool colvalid = (c >= 2) && (c < Np);
    const uint32_t vmask = colvalid ? rowvalid : 0u;
    // extended words: bit r+2 <-> row r; bits 0,1 <-> rows -2,-1 (from above)
    const uint32_t e0 = (w0 << 2) | h0.b;
    const uint32_t e1 = (w1 << 2) | h1.b;
    const uint32_t e2 = (w2 << 2) | h2.b;
    const uint32_t kc = key0 + (uint32_t)c;  // key of (row 0, c); only used where colvalid
    const float g_open = go, g_ext = ge;
    auto gam = [&](uint32_t bit) { return bit ? g_open : g_ext; };
    float cb = 0.0f;  // this column's first maximum and its key
    uint32_t ck = 0u;
    uint32_t word = 0u;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const float Qa = r >= 1 ? q1[r - 1] : h1.q31;                        // Q[r-1][c-1]
      float Qb = r >= 2 ? q1[r - 2] : (r == 1 ? h1.q31 : h1.q30);          // Q[r-2][c-1]
      float Qc = r >= 1 ? q2[r - 1] : h2.q31;                              // Q[r-1][c-2]
      if constexpr (ALIGN == 1) {
        Qb = Qb + (float)((e0 >> (r + 1)) & 1u);  // + C[r-1][c]
        Qc = Qc + (float)((e1 >> (r + 2)) & 1u);  // + C[r][c-1]
      }
      const bool hit = (e0 >> (r + 2)) & 1u;
      float pa = Qa, pb = Qb, pc = Qc;
      if (!EQG) {
        const float x = Qa - gam((e1 >> (r + 1)) & 1u);  // gamma(C[r-1][c-1])
        const float y = Qb - gam((e1 >> r) & 1u);        // gamma(C[r-2][c-1])
        const float z = Qc - gam((e2 >> (r + 1)) & 1u);  // gamma(C[r-1][c-2])
        pa = hit ? Qa : x;
        pb = hit ? Qb : y;
        pc = hit ? Qc : z;
      }
      float mx = pa;
      uint32_t k = 1u;
      if (pb > mx) {
        mx = pb;
        k = 2u;
      }
      if (pc > mx) {
        mx = pc;
        k = 3u;
      }
      float v = hit ? mx + 1.0f : fmaxf(EQG ? mx - g_open : mx, 0.0f);
      k = (hit && !(mx > 0.0f)) ? 0u : k;  // all predecessors 0: the path starts here
      v = ((vmask >> r) & 1u) ? v : 0.0f;
      k = v > 0.0f ? k : 0u;
      word |= k << (2 * r);
      // Pin the word row by row: it is first read at the store below, and left alone the compiler
      // sinks every code's selects there and carries their compare masks (a scalar register pair
      // each) across the row loop: 79 scalar spills at R = 16.
      asm volatile("" : "+v"(word));
      if (v > cb) {
        cb = v;
        ck = kc + ((uint32_t)r << 16);
      }
      qn[r] = v;
    }
    if (cb > best || (cb == best && cb > 0.0f && ck < bkey)) {
      best = cb;
      bkey = ck;
    }
    if (stores && c >= 0 && c < Np) drow[c] = (Word)word;
    DpAbove out;
    out.q30 = qn[R - 2];
    out.q31 = qn[R - 1];
    out.b = (w0 >> (R - 2)) & 3u;
    h2 = h1;
    h1 = h0;
    w2 = w1;
    w1 = w0;
    return out;
  }
};

// bnd: ceil(L / (64 R)) * ld float4 per pair, as the tracing DP's records are counted; plane:
// pstride bytes between pairs. qmax_out may be NULL.
template <int ALIGN, bool EQG, int R>
__global__ __launch_bounds__(64) void k_crp_dp_dir(const uint32_t* __restrict__ maskT, int64_t mask_stride, int ld,
                                                   const int2* __restrict__ dims, int row_lo, int row_hi, float go,
                                                   float ge, float4* __restrict__ bnd, int64_t bnd_stride,
                                                   uint8_t* __restrict__ plane, int64_t plane_stride,
                                                   uint32_t* __restrict__ endkey, float* __restrict__ qmax_out) {
  using Lane = DpLaneD<ALIGN, EQG, R>;
  using Word = typename Lane::Word;
  const int p = blockIdx.x;
  const int lane = threadIdx.x;
  const int2 dm = dims[p];
  const int Mp = dm.x, Np = dm.y;
  if (!(Mp > row_lo && Mp <= row_hi)) return;  // the other R's launch takes this pair (wave-uniform)
  const int nbands = (Mp + 64 * R - 1) / (64 * R);
  Word* const pl = reinterpret_cast<Word*>(plane + (size_t)p * plane_stride);
  Lane L;
  L.go = go;
  L.ge = ge;
  L.Np = Np;
  L.best = 0.0f;
  L.bkey = 0u;
  for (int band = 0; band < nbands; ++band) {
    const Band<Lane> B(p, band, nbands, lane, maskT, mask_stride, ld, bnd, bnd_stride);
    L.rowvalid = row_valid_mask<R>(B.row0, Mp);
    L.key0 = (uint32_t)B.row0 << 16;
    const bool lane_active = B.row0 < Mp;
    L.drow = pl + (size_t)(band * 64 + lane) * ld;
    L.stores = lane_active;
    dp_walk(L, B, lane, Np + 63, [&](int c) -> uint32_t {
      if (!(lane_active && c >= 0 && c < Np)) return 0u;
      return (B.mrow[c] >> B.sh) & ((1u << R) - 1u);
    });
    __threadfence_block();
    __syncthreads();
  }
  float best = L.best;
  uint32_t bkey = L.bkey;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float v = __shfl_xor(best, o);
    const uint32_t k = (uint32_t)__shfl_xor((int)bkey, o);
    if (v > best || (v == best && v > 0.0f && k < bkey)) {
      best = v;
      bkey = k;
    }
  }
  if (lane == 0) {
    if (qmax_out) qmax_out[p] = best;
    endkey[p] = best > 0.0f ? bkey : kNoEnd;
  }
}

// --------------------------------------------------------------------------------------
// k_crp_backtrack: one wave per pair. Lane 0 walks the direction plane from the end cell: note the
// cell, read its code, step to the predecessor, stop at code 0. The walk is a counted loop of at
// most min(M', N', path_cap) cells that also ends when a step would leave the matrix, so whatever
// the plane holds it ends and reads inside the pair's plane. The cells land in path[] last to
// first; then the whole wave turns them round in place and fills the rest of the pair's path_cap
// entries with -1. seg (unless NULL): the first and last cell, (-1, -1, -1, -1) for no path.
// --------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_crp_backtrack(const uint8_t* __restrict__ plane, int64_t plane_stride, int ld,
                                                      const int2* __restrict__ dims,
                                                      const uint32_t* __restrict__ endkey, int path_cap,
                                                      int32_t* __restrict__ seg_out, int32_t* __restrict__ len_out,
                                                      int32_t* path_out) {
  __shared__ int s_n;
  const int p = blockIdx.x;
  const int lane = threadIdx.x;
  int2* const out = reinterpret_cast<int2*>(path_out) + (size_t)p * path_cap;
  if (lane == 0) {
    const int2 dm = dims[p];
    const int Mp = dm.x, Np = dm.y;
    const uint32_t key = endkey[p];
    int i = (int)(key >> 16), j = (int)(key & 0xffffu);
    int n = 0, i0 = -1, j0 = -1, i1 = -1, j1 = -1;
    if (key != kNoEnd && i >= 2 && i < Mp && j >= 2 && j < Np) {
      const uint8_t* const pl = plane + (size_t)p * plane_stride;
      const bool r8 = Mp <= kTraceShortRows;
      const int lim = min(min(Mp, Np), path_cap);
      i1 = i;
      j1 = j;
      while (n < lim) {
        out[n++] = make_int2(i, j);
        i0 = i;
        j0 = j;
        uint32_t code;
        if (r8)
          code = reinterpret_cast<const uint16_t*>(pl)[(size_t)(i >> 3) * ld + j] >> (2 * (i & 7));
        else
          code = reinterpret_cast<const uint32_t*>(pl)[(size_t)(i >> 4) * ld + j] >> (2 * (i & 15));
        code &= 3u;
        if (code == 0u) break;
        i -= code == 2u ? 2 : 1;
        j -= code == 3u ? 2 : 1;
        if (i < 2 || j < 2) break;
      }
    }
    if (seg_out) {
      int32_t* sg = seg_out + 4 * (size_t)p;
      sg[0] = i0;
      sg[1] = j0;
      sg[2] = i1;
      sg[3] = j1;
    }
    len_out[p] = n;
    s_n = n;
  }
  __threadfence_block();
  __syncthreads();
  path_turn_and_pad(out, s_n, path_cap, lane);
}

// --------------------------------------------------------------------------------------
// k_crp_backtrack_dmax: the walk back over a chen17 plane (k_crp_dp_dir<1, ., .>). The code of a
// cell X names its predecessor P as before, but a b or c step also passed an intermediate cell I,
// (i-1, j) or (i, j-1), and P may score 0, where the path stops without it. Both are read off the
// pair's CRP words (strip-major, bit i & 31 of word (i >> 5) ld + j) and the plane:
//  * I is on the path where C[I] is set: it is the hit the bonus paid for;
//  * D[P] > 0 exactly where P lies in rows and columns >= 2 and is a hit (D >= 1) or a miss with a
//    code (a miss without one scores 0); the walk goes on at P then, and otherwise ends on I.
// Every cell the loop reads lies in [1, M') x [1, N'): X and a P it moves to in [2, M') x [2, N'),
// I one row or one column before X. It emits at most two cells per turn and tests the count,
// min(dmax_path_bound(M', N'), path_cap), before each, so whatever the plane holds it ends and
// writes inside the pair's path_cap entries. The code of P, C[P] and C[I] are three independent
// loads behind the code of X: one load of latency per step, as in k_crp_backtrack.
// --------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_crp_backtrack_dmax(const uint8_t* __restrict__ plane, int64_t plane_stride,
                                                           const uint32_t* __restrict__ maskT, int64_t mask_stride,
                                                           int ld, const int2* __restrict__ dims,
                                                           const uint32_t* __restrict__ endkey, int path_cap,
                                                           int32_t* __restrict__ seg_out,
                                                           int32_t* __restrict__ len_out, int32_t* path_out) {
  __shared__ int s_n;
  const int p = blockIdx.x;
  const int lane = threadIdx.x;
  int2* const out = reinterpret_cast<int2*>(path_out) + (size_t)p * path_cap;
  if (lane == 0) {
    const int2 dm = dims[p];
    const int Mp = dm.x, Np = dm.y;
    const uint32_t key = endkey[p];
    int i = (int)(key >> 16), j = (int)(key & 0xffffu);
    int n = 0, i0 = -1, j0 = -1, i1 = -1, j1 = -1;
    if (key != kNoEnd && i >= 2 && i < Mp && j >= 2 && j < Np) {
      const uint8_t* const pl = plane + (size_t)p * plane_stride;
      const uint32_t* const mk = maskT + (size_t)p * mask_stride;
      const bool r8 = Mp <= kTraceShortRows;
      const int lim = min(dmax_path_bound(Mp, Np), path_cap);
      auto code_at = [&](int a, int b) -> uint32_t {
        if (r8) return ((uint32_t) reinterpret_cast<const uint16_t*>(pl)[(size_t)(a >> 3) * ld + b] >> (2 * (a & 7))) & 3u;
        return (reinterpret_cast<const uint32_t*>(pl)[(size_t)(a >> 4) * ld + b] >> (2 * (a & 15))) & 3u;
      };
      auto crp_at = [&](int a, int b) -> uint32_t { return (mk[(size_t)(a >> 5) * ld + b] >> (a & 31)) & 1u; };
      i1 = i;
      j1 = j;
      uint32_t code = code_at(i, j);
      while (n < lim) {
        out[n++] = make_int2(i, j);
        i0 = i;
        j0 = j;
        if (code == 0u) break;
        const int pi = i - (code == 2u ? 2 : 1), pj = j - (code == 3u ? 2 : 1);
        const int ii = code == 2u ? i - 1 : i, ij = code == 3u ? j - 1 : j;  // I (X itself for code 1)
        const bool p_in = pi >= 2 && pj >= 2;
        const uint32_t pcode = p_in ? code_at(pi, pj) : 0u;
        const uint32_t phit = p_in ? crp_at(pi, pj) : 0u;
        if (code != 1u && crp_at(ii, ij)) {
          if (n >= lim) break;
          out[n++] = make_int2(ii, ij);
          i0 = ii;
          j0 = ij;
        }
        if (!(phit | pcode)) break;  // D[P] == 0: the path began on I
        i = pi;
        j = pj;
        code = pcode;
      }
    }
    if (seg_out) {
      int32_t* sg = seg_out + 4 * (size_t)p;
      sg[0] = i0;
      sg[1] = j0;
      sg[2] = i1;
      sg[3] = j1;
    }
    len_out[p] = n;
    s_n = n;
  }
  __threadfence_block();
  __syncthreads();
  path_turn_and_pad(out, s_n, path_cap, lane);
}

// --------------------------------------------------------------------------------------
// k_crp_rqa<R>: cross-recurrence quantification of a pair (the definition: include/acoss_hip.h,
// acoss_crp_rqa): the histogram H of its diagonal lines, folded by the same wave into n_rec, the
// line counts, lmax and RR, DET, LMEAN, ENTR. One wave per pair in bands, as k_crp_dp.
//  * DpLaneR keeps L[r][c], the length of the diagonal run that ends on (r, c): L[r-1][c-1] + 1 on
//    a hit, else 0. It depends on column c-1 only; what goes down a lane is the last row's L and the
//    CRP bits of the last three rows. All M' rows and N' columns count (no "rows and columns 0 and 1
//    hold 0" here): the fetch masks the words to the matrix and nothing else.
//  * a run is counted once, where it ends: at a miss inside the matrix whose up-left neighbour is
//    set (the run's length is that neighbour's L), and at once at a hit in the last row or the last
//    column (its own L): no virtual row below a full last band, no column N'.
//  * nearly all runs are short, so the two hottest bins never see an atomic: with e_k = "bit r is
//    C[r-k][c-k]" (the words of columns c-1, c-2, c-3 shifted by 1, 2, 3 rows, the rows from above
//    spliced in), a run of length 1 ends where e_1 & ~e_2, one of length 2 where e_1 & e_2 & ~e_3
//    (at an edge hit: ~e_1, and e_1 & ~e_2): two popcounts per column into lane registers, summed
//    over the wave once. Only runs of 3 cells and more go to the pair's LDS histogram (dynamic,
//    nbins counters), by an atomic add under a branch most steps skip.
//  * n_rec is the popcount of the masked words.
// The fold: lane t takes the bins t, t + 64, ... in ascending order, integers exactly; ENTR in
// float64, -p ln p summed per lane in that order and then over the lanes by the xor butterfly
// (32, 16, ..., 1): one fixed order.
// --------------------------------------------------------------------------------------
struct DpAboveR {  // what lane l-1 (or the band above) hands down for one column
  uint32_t l;      // L of its last row
  uint32_t b;      // bit0 = C[row R-3], bit1 = C[row R-2], bit2 = C[row R-1]
};

template <int R>
struct DpLaneR {
  static constexpr int kRows = R;
  using Above = DpAboveR;
  using Rec = uint2;  // l, b
  using Col = uint32_t[R];  // one column: the run length that ends on each of this lane's rows
  static __device__ __forceinline__ Above shfl_up(const Above& a) {
    return Above{(uint32_t)__shfl_up((int)a.l, 1), (uint32_t)__shfl_up((int)a.b, 1)};
  }
  static __device__ __forceinline__ Above from_rec(const Rec& v) { return Above{v.x, v.y}; }
  static __device__ __forceinline__ Rec to_rec(const Above& o) { return make_uint2(o.l, o.b); }

  int Np;
  uint32_t rin;         // bit r: global row < Mp
  uint32_t lastrow;     // bit r: global row == Mp - 1
  uint32_t w1, w2, w3;  // CRP words of columns c-1, c-2, c-3 (bit r = row r)
  DpAboveR h1, h2, h3;  // from above for the same columns
  uint32_t n_rec, n1, n2;  // set cells, runs of length 1 and of length 2 that this lane saw end
  uint32_t* hist;       // the pair's LDS histogram and its last bin
  uint32_t maxbin;

  __device__ __forceinline__ DpAboveR step(Col& qn, const Col& q1, const Col&, uint32_t w0, const DpAboveR& h0, int c) {
    // bit r of e_k: C[r-k][c-k]; a neighbour outside the matrix reads 0 (the fetch, the top edge)
    const uint32_t e1 = (w1 << 1) | (h1.b >> 2);
    const uint32_t e2 = (w2 << 2) | (h2.b >> 1);
    const uint32_t e3 = (w3 << 3) | h3.b;
    const bool incol = c >= 0 && c < Np;
    const uint32_t ends = e1 & ~w0 & (incol ? rin : 0u);       // misses that end a run
    const uint32_t edge = w0 & (c == Np - 1 ? rin : lastrow);  // hits no cell can follow
    n_rec += __builtin_popcount(w0);
    n1 += __builtin_popcount((ends & ~e2) | (edge & ~e1));
    n2 += __builtin_popcount((ends & e2 & ~e3) | (edge & e1 & ~e2));
    const uint32_t lng = (ends & e2 & e3) | (edge & e1 & e2);  // runs of 3 cells and more
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const uint32_t prev = r >= 1 ? q1[r - 1] : h1.l;
      qn[r] = ((w0 >> r) & 1u) ? prev + 1u : 0u;
    }
    if (lng) {
#pragma unroll
      for (int r = 0; r < R; ++r) {
        if ((lng >> r) & 1u) {
          const uint32_t prev = r >= 1 ? q1[r - 1] : h1.l;
          atomicAdd(&hist[min(max(qn[r], prev), maxbin)], 1u);  // prev at a miss, prev + 1 at an edge hit
        }
      }
    }
    DpAboveR out;
    out.l = qn[R - 1];
    out.b = (w0 >> (R - 3)) & 7u;
    h3 = h2;
    h2 = h1;
    h1 = h0;
    w3 = w2;
    w2 = w1;
    w1 = w0;
    return out;
  }
};

__device__ __forceinline__ int64_t wave_sum_i64(int64_t v) {  // the total in every lane
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += (int64_t)__shfl_xor((long long)v, o);
  return v;
}

// bnd: ceil(L / 2048) * ld records per pair (only CRPs of more than one band touch them); dynamic
// LDS: nbins counters, nbins - 1 >= min(M', N') of every pair. counts (4 per pair: n_rec, n_lines,
// n_lines_min, n_pts_min), lmax, stats (4 per pair: RR, DET, LMEAN, ENTR) and hist (hist_cap per
// pair) may each be NULL.
template <int R>
__global__ __launch_bounds__(64) void k_crp_rqa(const uint32_t* __restrict__ maskT, int64_t mask_stride, int ld,
                                                const int2* __restrict__ dims, int lmin, int nbins,
                                                uint2* __restrict__ bnd, int64_t bnd_stride,
                                                int64_t* __restrict__ counts, int32_t* __restrict__ lmax_out,
                                                double* __restrict__ stats, int hist_cap,
                                                int32_t* __restrict__ hist_out) {
  using Lane = DpLaneR<R>;
  extern __shared__ uint32_t s_hist[];
  const int p = blockIdx.x;
  const int lane = threadIdx.x;
  const int2 dm = dims[p];
  const int Mp = dm.x, Np = dm.y;
  for (int t = lane; t < nbins; t += 64) s_hist[t] = 0u;
  __syncthreads();
  const int nbands = (Mp > 0 && Np > 0) ? (Mp + 64 * R - 1) / (64 * R) : 0;
  Lane L;
  L.Np = Np;
  L.n_rec = L.n1 = L.n2 = 0u;
  L.hist = s_hist;
  L.maxbin = (uint32_t)(nbins - 1);
  for (int band = 0; band < nbands; ++band) {
    const Band<Lane> B(p, band, nbands, lane, maskT, mask_stride, ld, bnd, bnd_stride);
    const int left = Mp - B.row0;  // rows of the matrix from this lane's first one on
    const int own = left < 0 ? 0 : (left < R ? left : R);  // how many of them are this lane's
    const uint32_t rin = L.rin = own >= 32 ? 0xffffffffu : (1u << own) - 1u;
    L.lastrow = (left >= 1 && left <= R) ? 1u << (left - 1) : 0u;
    L.w3 = 0u;
    L.h3 = DpAboveR{};
    dp_walk(L, B, lane, Np + 63, [&](int c) -> uint32_t {
      if (!(rin != 0u && c >= 0 && c < Np)) return 0u;
      return (B.mrow[c] >> B.sh) & rin;
    });
    __threadfence_block();
    __syncthreads();
  }
  const int64_t n_rec = wave_sum_i64((int64_t)L.n_rec);
  const int64_t h1 = wave_sum_i64((int64_t)L.n1), h2 = wave_sum_i64((int64_t)L.n2);
  if (lane == 0) {
    if (nbins > 1) s_hist[1] += (uint32_t)h1;
    if (nbins > 2) s_hist[2] += (uint32_t)h2;
  }
  __syncthreads();
  const int lim = min(min(Mp, Np), nbins - 1);  // the longest line the pair can hold
  int64_t nl = 0, nlm = 0, npm = 0;
  int lm = 0;
  for (int l = 1 + lane; l <= lim; l += 64) {
    const int64_t h = (int64_t)s_hist[l];
    nl += h;
    if (l >= lmin) {
      nlm += h;
      npm += h * l;
    }
    if (h > 0) lm = l;
  }
  nl = wave_sum_i64(nl);
  nlm = wave_sum_i64(nlm);
  npm = wave_sum_i64(npm);
  lm = (int)wave_max_u32((unsigned)lm);
  if (hist_out) {
    int32_t* const ho = hist_out + (size_t)p * hist_cap;
    for (int l = lane; l < hist_cap; l += 64) ho[l] = (l >= 1 && l <= lim) ? (int32_t)s_hist[l] : 0;
  }
  if (stats) {  // wave-uniform
    double e = 0.0;
    if (nlm > 0) {
      const double tot = (double)nlm;
      for (int l = 1 + lane; l <= lim; l += 64) {
        const uint32_t h = s_hist[l];
        if (l >= lmin && h > 0u) {
          const double pl = (double)h / tot;
          e -= pl * log(pl);
        }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) e += __shfl_xor(e, o);
    }
    if (lane == 0) {
      double* st = stats + 4 * (size_t)p;
      const double cells = (double)Mp * (double)Np;
      st[0] = cells > 0.0 ? (double)n_rec / cells : 0.0;
      st[1] = n_rec > 0 ? (double)npm / (double)n_rec : 0.0;
      st[2] = nlm > 0 ? (double)npm / (double)nlm : 0.0;
      st[3] = e;
    }
  }
  if (lane == 0) {
    if (counts) {
      int64_t* ct = counts + 4 * (size_t)p;
      ct[0] = n_rec;
      ct[1] = nl;
      ct[2] = nlm;
      ct[3] = npm;
    }
    if (lmax_out) lmax_out[p] = lm;
  }
}

// --------------------------------------------------------------------------------------
// Which kernel runs
// --------------------------------------------------------------------------------------
namespace {

// gamma = K/2 with 0 <= K <= 1024: with equal gammas every score is an exact multiple of 1/2, what
// the FAST step, the grouped and the packed kernel and the tracing DP's single select rest on
inline bool half_integer_gamma(float g) {
  const float k2 = 2.0f * g;
  return k2 >= 0.0f && k2 <= 1024.0f && k2 == floorf(k2);
}

template <int ALIGN, int R>
void launch_dp_r(bool eqg, int nb, const uint32_t* maskT, int64_t mstride, int ld, const int2* dims, float go,
                 float ge, float4* bnd, int64_t bstride, float* out, hipStream_t s, int L = 0) {
  static const bool no_fast = getenv("ACOSS_DP_NOFAST") != nullptr;
  static const bool no_grp = getenv("ACOSS_DP_NOGROUP") != nullptr;
  const bool fast = ALIGN == 0 && eqg && !no_fast && half_integer_gamma(go);
  const int LP = (L + 31) / 32;  // lanes per pair at 32 rows per lane
  auto wave_per_pair = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3(nb), dim3(64), 0, s, maskT, mstride, ld, dims, go, ge, bnd, bstride, out);
  };
  if (fast && !no_grp && L > 0 && LP <= 21) {  // three or more pairs per wave (two per wave measured slower at L ~ 1000)
    const int G = 64 / LP;
    hipLaunchKernelGGL(k_crp_dp_grp, dim3((unsigned)((nb + G - 1) / G)), dim3(64), 0, s, maskT, mstride, ld, dims, nb,
                       LP, go, out);
  } else if (fast)
    wave_per_pair(k_crp_dp_fast<R>);
  else if (eqg)
    wave_per_pair(k_crp_dp<ALIGN, true, R>);
  else
    wave_per_pair(k_crp_dp<ALIGN, false, R>);
}

// The packed 16-bit DP (k_crp_dp_pk) is exact when gamma_open == gamma_ext is a multiple of 1/2
// and every doubled score fits 16 bits: scores grow by at most 2 per column (chen17), so 2Q < 4L.
inline bool dp_packed_ok(bool eqg, int L, float go) {
  static const bool off = getenv("ACOSS_DP_F32") != nullptr;
  return !off && eqg && L <= 16000 && half_integer_gamma(go);
}

// Rows per lane from the batch's longest CRP (L rows): every choice below 2048 rows is one band,
// so the band-boundary buffer (ceil(L / 2048) bands) always suffices.
template <int ALIGN>
void launch_dp_a(bool eqg, int nb, int L, const uint32_t* maskT, int64_t mstride, int ld, const int2* dims, float go,
                 float ge, float4* bnd, int64_t bstride, float* out, hipStream_t s) {
  if (L <= 512)
    launch_dp_r<ALIGN, 8>(eqg, nb, maskT, mstride, ld, dims, go, ge, bnd, bstride, out, s, L);
  else if (L <= 1024)
    launch_dp_r<ALIGN, 16>(eqg, nb, maskT, mstride, ld, dims, go, ge, bnd, bstride, out, s, L);
  else {
    if constexpr (ALIGN == 1) {  // chen17 only: k_crp_dp_pk<0> is never instantiated
      if (dp_packed_ok(eqg, L, go)) {
        hipLaunchKernelGGL(k_crp_dp_pk<1>, dim3(nb), dim3(64), 0, s, maskT, mstride, ld, dims, (unsigned)(2.0f * go),
                           bnd, bstride, out);
        return;
      }
    }
    launch_dp_r<ALIGN, 32>(eqg, nb, maskT, mstride, ld, dims, go, ge, bnd, bstride, out, s);
  }
}

// The tracing DP (k_crp_dp_trace): R = 8 takes the CRPs of at most 512 rows, R = 16 the longer
// ones; a batch whose longest CRP has more than 512 rows gets both launches and each wave keeps
// the pairs of its own R. The exact-halves select (EQG) under the fast DP's condition only. The
// direction DP (k_crp_dp_dir) is launched the same way: launch(R as a type, halves, row_lo, row_hi)
// names the kernel.
template <class Launch>
void launch_by_rows(int L, float go, float ge, Launch launch) {
  const bool halves = go == ge && half_integer_gamma(go);
  launch(std::integral_constant<int, 8>{}, halves, -1, kTraceShortRows);
  if (L > kTraceShortRows) launch(std::integral_constant<int, 16>{}, halves, kTraceShortRows, INT32_MAX);
}

}  // namespace

void launch_dp(int align, bool eqg, int nb, int L, const uint32_t* maskT, int64_t mstride, int ld, const int2* dims,
               float go, float ge, float4* bnd, int64_t bstride, float* out, hipStream_t s) {
  if (align == 0)
    launch_dp_a<0>(eqg, nb, L, maskT, mstride, ld, dims, go, ge, bnd, bstride, out, s);
  else
    launch_dp_a<1>(eqg, nb, L, maskT, mstride, ld, dims, go, ge, bnd, bstride, out, s);
}

int64_t trace_bnd_records(int L, int ld) {  // per pair: ceil(L / (64 R)) * ld
  return L <= kTraceShortRows ? (int64_t)ld : (int64_t)((L + 64 * 16 - 1) / (64 * 16)) * ld;
}

void launch_trace(int align, int nb, int L, const uint32_t* maskT, int64_t mstride, int ld, const int2* dims, float go,
                  float ge, void* bnd, int64_t bstride, float* score, int32_t* seg, hipStream_t s) {
  launch_by_rows(L, go, ge, [&](auto r, bool halves, int row_lo, int row_hi) {
    constexpr int R = decltype(r)::value;
    auto launch = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, dim3(nb), dim3(64), 0, s, maskT, mstride, ld, dims, row_lo, row_hi, go, ge,
                         static_cast<TraceRec*>(bnd), bstride, score, seg);
    };
    if (align == 0)
      launch(halves ? k_crp_dp_trace<0, true, R> : k_crp_dp_trace<0, false, R>);
    else
      launch(halves ? k_crp_dp_trace<1, true, R> : k_crp_dp_trace<1, false, R>);
  });
}

// per pair: ceil(L / 16) row groups of ld 32-bit words; the 16-bit words of the 8-row groups of a
// CRP of at most 512 rows never take more
int64_t dir_plane_bytes(int L, int ld) { return (int64_t)((L + 15) / 16) * ld * 4; }

void launch_dir(int align, int nb, int L, const uint32_t* maskT, int64_t mstride, int ld, const int2* dims, float go,
                float ge, float4* bnd, int64_t bstride, uint8_t* plane, int64_t pstride, uint32_t* endkey, float* score,
                hipStream_t s) {
  launch_by_rows(L, go, ge, [&](auto r, bool halves, int row_lo, int row_hi) {
    constexpr int R = decltype(r)::value;
    auto launch = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, dim3(nb), dim3(64), 0, s, maskT, mstride, ld, dims, row_lo, row_hi, go, ge, bnd,
                         bstride, plane, pstride, endkey, score);
    };
    if (align == 0)
      launch(halves ? k_crp_dp_dir<0, true, R> : k_crp_dp_dir<0, false, R>);
    else
      launch(halves ? k_crp_dp_dir<1, true, R> : k_crp_dp_dir<1, false, R>);
  });
}

void launch_backtrack(int align, int nb, const uint8_t* plane, int64_t pstride, const uint32_t* maskT, int64_t mstride,
                      int ld, const int2* dims, const uint32_t* endkey, int path_cap, int32_t* seg, int32_t* len,
                      int32_t* path, hipStream_t s) {
  if (align == 0)
    hipLaunchKernelGGL(k_crp_backtrack, dim3(nb), dim3(64), 0, s, plane, pstride, ld, dims, endkey, path_cap, seg, len,
                       path);
  else
    hipLaunchKernelGGL(k_crp_backtrack_dmax, dim3(nb), dim3(64), 0, s, plane, pstride, maskT, mstride, ld, dims, endkey,
                       path_cap, seg, len, path);
}

int64_t rqa_bnd_records(int L, int ld) { return (int64_t)((L + 2047) / 2048) * ld; }

void launch_rqa(int nb, int L, int nbins, const uint32_t* maskT, int64_t mstride, int ld, const int2* dims, int lmin,
                void* bnd, int64_t bstride, int64_t* counts, int32_t* lmax, double* stats, int hist_cap, int32_t* hist,
                hipStream_t s) {
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3(nb), dim3(64), sizeof(uint32_t) * (size_t)nbins, s, maskT, mstride, ld, dims, lmin,
                       nbins, static_cast<uint2*>(bnd), bstride, counts, lmax, stats, hist_cap, hist);
  };
  // rows per lane as launch_dp's: one band up to 2048 rows
  if (L <= 512)
    launch(k_crp_rqa<8>);
  else if (L <= 1024)
    launch(k_crp_rqa<16>);
  else
    launch(k_crp_rqa<32>);
}

}  // namespace acoss
