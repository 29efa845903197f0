// sw.hip — smith_waterman_constrained (acoss/algorithms/utils/alignment_tools.py:7-46) in float64,
// and where its alignment lies: acoss_sw_constrained, acoss_sw_locate, acoss_sw_path, and through
// sw_internal.hpp the four matrices of every EarlyFusion and early-SNF pair. The definition of the
// located and traced alignment is in include/acoss_hip.h (acoss_sw_locate); tests/sw_path_np.py
// restates it in numpy. Six kernels around one cell; the scoring ones share one wavefront walk.
//
// The binary matrix arrives as a bit plane: word W[g][c] (u16) holds rows 16 g .. 16 g + 15 of
// column c. A chain of lanes owns consecutive rows (R each) and sweeps the columns skewed by one per
// lane, reading one word per column (prefetched four columns ahead); the last rows of a lane (2 of
// S, 3 of B) pass down one lane per step with __shfl_up; where a matrix has more rows than a wave
// covers, bands of 64 R rows chain through HBM records.
//   S[i][j] = max((S[i-1][j-1] + m) + d(B[i-2][j-2]), (S[i-2][j-1] + m) + d(B[i-3][j-2]),
//                 (S[i-1][j-2] + m) + d(B[i-2][j-3]), 0),  i, j >= 3,
//   m = B[i-1][j-1] ? 1 : -1,  d(v) = v > 0 ? 0 : -0.7
// sw_cell is that cell, written once. sw_walk is that walk under the scoring kernels; as in
// crp_dp.hip, what differs between them is passed to the walk:
//  * a lane policy: what a lane keeps per column and the recurrence on it (step).
//      SwLane<R>     scores only: the lane's maximum
//  * an edge policy: what is above the chain's first lane and below its last one.
//      SwBand       the band above / below, through HBM records
//      SwGroupEdge  nothing above, nothing kept
//  * the lane's index in its chain, the number of steps (wave-uniform) and the fetch of a column's word.
//
//  k_swb<8>, k_swb<16>  scores, one matrix per wave in bands of 64 R rows. R = 8 when the batch's
//                       matrices have <= 512 rows (56 of 64 lanes busy at 446 rows), else 16.
//  k_swb_grp            scores of small matrices (at most 256 rows: EarlyFusion's beat-block CSMs,
//                       M ~ 14..47): a chain of LP <= 32 lanes per matrix at 8 rows per lane, G = 64 /
//                       LP matrices per wave instead of one with most lanes idle, one band each.
//  k_swt<false>, k_swt<true>  the tracing and the direction DP at 8 rows per lane, for every shape
//                       launch_swb_batch serves: LP <= 32 as k_swb_grp lays the matrices out, LP = 64
//                       one matrix per wave in bands of 512 rows. Beside every S the tracing DP
//                       keeps the packed cell (r0 << 16) | c0 where its path began; the direction
//                       DP writes a 2-bit predecessor code per cell to a plane. Its own loop over
//                       sw_cell, for its time.
//  k_sw_backtrack       the walk back over the direction DP's plane
// Every kernel's scores are the same cell in the same order, so they are equal bit for bit. Cells
// are named in the binary matrix's own coordinates: the walk's row i and column c (those of the
// reference's score matrix) are the cell (i - 1, c - 1).
#include <algorithm>

#include "sw_internal.hpp"

namespace acoss {

namespace {

constexpr int kR = 8;  // rows per lane of the tracing and direction DP, and of k_swb_grp
constexpr uint32_t kSwNoEnd = 0xffffffffu;

// --------------------------------------------------------------------------------------
// The cell.
// --------------------------------------------------------------------------------------
struct SwAbove {  // what the lane above (or the band above) hands down for one column
  double sa, sb;  // S of its rows R-2, R-1
  uint32_t b;     // B bits of its rows R-3, R-2, R-1 (bits 0..2)
};

struct SwCell {
  double v;    // S of the cell
  double ps;   // S of the chosen predecessor: the first of a, b, c that attains the maximum
  uint32_t k;  // and its index, 1 / 2 / 3
};

// Row r of a lane at column c. s1, s2: the lane's columns c-1, c-2; h1, h2: from above for those
// columns; e1..e3: the extended bit words of columns c-1..c-3 (bit r+3 <-> my row r; bits 0..2 <->
// rows -3..-1); scored: the cell lies in rows and columns [3, M) x [3, N) of the walk. A lane that
// only wants the value leaves ps and k unread, and nothing of them is left in its code.
template <int R>
__device__ __forceinline__ SwCell sw_cell(const double (&s1)[R], const double (&s2)[R], const SwAbove& h1,
                                          const SwAbove& h2, uint32_t e1, uint32_t e2, uint32_t e3, int r,
                                          bool scored) {
  const double A = r >= 1 ? s1[r - 1] : h1.sb;                      // S[i-1][c-1]
  const double Bv = r >= 2 ? s1[r - 2] : (r == 1 ? h1.sb : h1.sa);  // S[i-2][c-1]
  const double Cv = r >= 1 ? s2[r - 1] : h2.sb;                     // S[i-1][c-2]
  const double mv = ((e1 >> (r + 2)) & 1) ? 1.0 : -1.0;             // B[i-1][c-1]
  const double d1 = ((e2 >> (r + 1)) & 1) ? 0.0 : -0.7;             // B[i-2][c-2]
  const double d2 = ((e2 >> r) & 1) ? 0.0 : -0.7;                   // B[i-3][c-2]
  const double d3 = ((e3 >> (r + 1)) & 1) ? 0.0 : -0.7;             // B[i-2][c-3]
  const double x1 = (A + mv) + d1;
  const double x2 = (Bv + mv) + d2;
  const double x3 = (Cv + mv) + d3;
  SwCell o{x1, A, 1u};
  if (x2 > o.v) o = SwCell{x2, Bv, 2u};
  if (x3 > o.v) o = SwCell{x3, Cv, 3u};
  o.v = 0.0 > o.v ? 0.0 : o.v;
  o.v = scored ? o.v : 0.0;
  return o;
}

// --------------------------------------------------------------------------------------
// The walk.
//   Lane:  Above (what goes down one lane per column; Above{} = nothing above), shfl_up(Above),
//          begin() (an empty history), step(w0, h0, c) -> Above, N.
//   Edge:  above(h, c, incol): h as shuffled, or what the edge supplies for the chain's first
//          lane; below(o, c, incol): keeps o where the chain's last lane has rows below it. Both
//          get the walk's one test of the column, incol = 0 <= c < N, and hold whatever does not
//          change from step to step ready-made.
//   fetch: word of column c restricted to this lane's rows (0 outside the matrix).
// --------------------------------------------------------------------------------------
template <class Lane, class Edge, class Fetch>
__device__ __forceinline__ void sw_walk(Lane& L, const Edge& E, int idx, int S_end, Fetch fetch) {
  using Above = typename Lane::Above;
  L.begin();
  Above pub{};  // what this lane hands down, one step late
  uint32_t q0 = fetch(-idx), q1 = fetch(1 - idx), q2 = fetch(2 - idx), q3 = fetch(3 - idx);
  for (int s = 0; s < S_end; ++s) {
    const int c = s - idx;
    const uint32_t w0 = q0;
    q0 = q1;
    q1 = q2;
    q2 = q3;
    q3 = fetch(c + 4);
    const bool incol = c >= 0 && c < L.N;
    const Above h0 = E.above(Lane::shfl_up(pub), c, incol);
    pub = L.step(w0, h0, c);
    E.below(pub, c, incol);
  }
}

// The boundary records of band `band` of matrix mid (N records per band): the chain's first lane
// reads the band above, its last lane writes for the band below.
template <class Lane>
struct SwBand {
  using Above = typename Lane::Above;
  using Rec = typename Lane::Rec;
  const Rec* bin;
  Rec* bout;
  bool first, reads, writes;  // the first lane; it, with a band above; the last lane, with a band below

  __device__ __forceinline__ SwBand(Rec* bnd, int N, int band, int nbands, int idx, int chain)
      : bin(bnd + (size_t)(band - 1) * N), bout(bnd + (size_t)band * N), first(idx == 0),
        reads(idx == 0 && band > 0), writes(idx == chain - 1 && band + 1 < nbands) {}
  __device__ __forceinline__ Above above(Above h, int c, bool incol) const {
    if (first) {  // by value and assigned: a choice between h and a record is a choice of addresses
      h = Above{};
      if (reads && incol) h = Lane::from_rec(bin[c]);
    }
    return h;
  }
  __device__ __forceinline__ void below(const Above& o, int c, bool incol) const {
    if (writes && incol) bout[c] = Lane::to_rec(o);
  }
};

// A group of lanes that holds all rows of its matrix: its first lane has nothing above.
template <class Lane>
struct SwGroupEdge {
  using Above = typename Lane::Above;
  bool first;
  __device__ __forceinline__ Above above(const Above& h, int, bool) const { return first ? Above{} : h; }
  __device__ __forceinline__ void below(const Above&, int, bool) const {}
};

// --------------------------------------------------------------------------------------
// The lane. SwCols is what it keeps: two columns of scores, three of bits, and what came from
// above for the same columns.
// --------------------------------------------------------------------------------------
template <int R>
struct SwCols {
  // a lane hands down rows R-2, R-1 of S and R-3 .. R-1 of the bits; a word holds 16 rows
  static_assert(R >= 3 && R <= 16 && 16 % R == 0, "rows per lane");
  int M, N, row0;         // the matrix, and this lane's first row in it
  double s1[R], s2[R];    // columns c-1, c-2
  uint32_t w1, w2, w3;    // B bits of my rows at c-1, c-2, c-3
  SwAbove h1, h2, h3;     // from above for the same columns

  __device__ __forceinline__ void begin() {
#pragma unroll
    for (int r = 0; r < R; ++r) s1[r] = s2[r] = 0.0;
    w1 = w2 = w3 = 0;
    h1 = h2 = h3 = SwAbove{};
  }
  // cok: 3 <= c < N, tested once per step
  __device__ __forceinline__ SwCell cell(int r, bool cok, uint32_t e1, uint32_t e2, uint32_t e3) const {
    const int i = row0 + r;
    return sw_cell<R>(s1, s2, h1, h2, e1, e2, e3, r, cok && i >= 3 && i < M);
  }
  // column c becomes column c-1; returns the scores and bits to hand down
  __device__ __forceinline__ SwAbove rotate(const double (&s0)[R], uint32_t w0, const SwAbove& h0) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      s2[r] = s1[r];
      s1[r] = s0[r];
    }
    w3 = w2;
    w2 = w1;
    w1 = w0;
    h3 = h2;
    h2 = h1;
    h1 = h0;
    return SwAbove{s0[R - 2], s0[R - 1], (w0 >> (R - 3)) & 7u};
  }
};

__device__ __forceinline__ SwAbove sw_shfl_up(const SwAbove& a) {
  return SwAbove{__shfl_up(a.sa, 1), __shfl_up(a.sb, 1), (uint32_t)__shfl_up((int)a.b, 1)};
}

template <int R>
struct SwLane : SwCols<R> {
  using Above = SwAbove;
  using Rec = double4;  // sa, sb, bits as double, unused
  static __device__ __forceinline__ Above shfl_up(const Above& a) { return sw_shfl_up(a); }
  static __device__ __forceinline__ Above from_rec(const Rec& v) { return Above{v.x, v.y, (uint32_t)v.z}; }
  static __device__ __forceinline__ Rec to_rec(const Above& o) { return make_double4(o.sa, o.sb, (double)o.b, 0.0); }

  double best;

  __device__ __forceinline__ Above step(uint32_t w0, const Above& h0, int c) {
    const uint32_t e1 = (this->w1 << 3) | this->h1.b;
    const uint32_t e2 = (this->w2 << 3) | this->h2.b;
    const uint32_t e3 = (this->w3 << 3) | this->h3.b;
    const bool cok = c >= 3 && c < this->N;
    double s0[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const double v = this->cell(r, cok, e1, e2, e3).v;
      best = v > best ? v : best;
      s0[r] = v;
    }
    return this->rotate(s0, w0, h0);
  }
};

struct SwAboveT : SwAbove {
  uint32_t oa, ob;  // origins of the cells sa, sb (tracing DP only)
};

struct SwtRec {  // one column of a band boundary of the tracing or direction DP
  double sa, sb;
  uint32_t b, oa, ob, unused;
};
static_assert(sizeof(SwtRec) == 32, "swt_bnd_bytes counts 32-byte records");

// Where band `band` of a matrix lies for lane idx of a chain of `chain` lanes at R rows per lane,
// and the fetch of its words.
template <int R>
struct SwRows {
  int row0, sh;
  const uint16_t* wr;
  bool rows_ok;
  int N;
  __device__ __forceinline__ SwRows(const uint16_t* Wm, int ldw, int band, int chain, int idx, bool live, int M,
                                    int N_)
      : row0((band * chain + idx) * R), sh(row0 & 15), wr(Wm + (size_t)(row0 >> 4) * ldw),
        rows_ok(live && row0 < M), N(N_) {}
  __device__ __forceinline__ uint32_t operator()(int c) const {
    return (rows_ok && c >= 0 && c < N) ? (((uint32_t)wr[c] >> sh) & ((1u << R) - 1)) : 0u;
  }
};

// --------------------------------------------------------------------------------------
// The kernels.
// --------------------------------------------------------------------------------------
template <int R>
__global__ __launch_bounds__(64) void k_swb(const uint16_t* __restrict__ W, int64_t wstride, int ldw,
                                            const int32_t* __restrict__ rows, const int32_t* __restrict__ cols,
                                            double4* __restrict__ bnd, int64_t bnd_stride, double* __restrict__ out) {
  static_assert(R == 8 || R == 16, "rows per lane");
  using Lane = SwLane<R>;
  const int mid = blockIdx.x;
  const int lane = threadIdx.x;
  const int M = rows[mid], N = cols[mid];
  if (M < 4 || N < 4) {
    if (lane == 0) out[mid] = 0.0;
    return;
  }
  const int nbands = (M + 64 * R - 1) / (64 * R);
  Lane L;
  L.M = M;
  L.N = N;
  L.best = 0.0;
  for (int band = 0; band < nbands; ++band) {
    const SwRows<R> rw(W + (size_t)mid * wstride, ldw, band, 64, lane, true, M, N);
    L.row0 = rw.row0;
    const int lanes = min(64, (M - band * 64 * R + R - 1) / R);  // lanes holding rows of this band
    sw_walk(L, SwBand<Lane>(bnd + (size_t)mid * bnd_stride, N, band, nbands, lane, 64), lane, N + lanes - 1, rw);
    __threadfence_block();
    __syncthreads();
  }
  const double best = wave_max(L.best);
  if (lane == 0) out[mid] = best;
}

// The chain a lane belongs to where G = 64 / LP matrices share a wave (G = 1: the whole wave).
struct SwChain {
  int ll, mid;  // the lane's index in its chain, and the chain's matrix
  bool in_group;
  __device__ __forceinline__ SwChain(int lane, int LP, int n) {
    const int G = 64 / LP, g = lane / LP;
    ll = lane - g * LP;
    mid = blockIdx.x * G + g;
    in_group = g < G && mid < n;
  }
};

__global__ __launch_bounds__(64) void k_swb_grp(const uint16_t* __restrict__ W, int64_t wstride, int ldw,
                                                const int32_t* __restrict__ rows, const int32_t* __restrict__ cols,
                                                int n, int LP, double* __restrict__ out) {
  using Lane = SwLane<kR>;
  __shared__ double s_best[64];
  const int lane = threadIdx.x;
  const SwChain C(lane, LP, n);
  const int M = C.in_group ? rows[C.mid] : 0, N = C.in_group ? cols[C.mid] : 0;
  const bool live = C.in_group && M >= 4 && N >= 4;
  const SwRows<kR> rw(W + (size_t)(C.in_group ? C.mid : 0) * wstride, ldw, 0, LP, C.ll, live, M, N);
  Lane L;
  L.M = M;
  L.N = N;
  L.row0 = rw.row0;
  L.best = 0.0;
  // steps until every group of the wave is done (wave-uniform bound)
  const int S_end = (int)wave_max_u32(live ? (unsigned)(N + LP - 1) : 0u);
  sw_walk(L, SwGroupEdge<Lane>{C.ll == 0}, C.ll, S_end, rw);
  // per-group maximum through LDS (groups need not be a power of two wide)
  s_best[lane] = L.best;
  __syncthreads();
  if (C.in_group && C.ll == 0) {
    double m = 0.0;
    for (int k = 0; k < LP; ++k) m = s_best[lane + k] > m ? s_best[lane + k] : m;
    out[C.mid] = live ? m : 0.0;
  }
}

// plane of a matrix: row groups of 8 rows of the walk (row i in group i >> 3, bits 2 (i & 7) and
// the next), ldp 16-bit words each, one per column of the walk
__host__ __device__ inline int swt_plane_pitch(int max_cols) { return (int)align_up((size_t)max_cols, 4); }

// Where the alignment lies. Beside the scores a lane keeps (best, end key) by the rule "among equal
// scores the smaller key" (the skewed walk does not visit cells in row-major order), and
//   DIR = false: an origin per cell, o1 / o2 as s1 / s2, handed down and across bands with the scores,
//                and the origin of its best cell;
//   DIR = true:  nothing more: the codes of a column go to the plane as one 16-bit word.
// This kernel keeps its own loop around sw_cell: as two lane policies on sw_walk it measured above
// the written-out loop's time in every phase on both EarlyFusion shapes. profiles/sw_walk/resources.md
// has the figures, and those of this form.
template <bool DIR>
__global__ __launch_bounds__(64) void k_swt(const uint16_t* __restrict__ W, int64_t wstride, int ldw,
                                            const int32_t* __restrict__ rows, const int32_t* __restrict__ cols, int n,
                                            int LP, SwtRec* __restrict__ bnd, int64_t bnd_stride,
                                            uint16_t* __restrict__ plane, int64_t plane_stride, int ldp,
                                            double* __restrict__ score_out, int32_t* __restrict__ seg_out,
                                            uint32_t* __restrict__ endkey) {
  constexpr int R = kR;
  constexpr unsigned kMask = (1u << R) - 1;
  __shared__ double s_best[64];
  __shared__ uint32_t s_key[64], s_org[64];
  const int lane = threadIdx.x;
  const SwChain C(lane, LP, n);
  const int ll = C.ll, mid = C.mid;
  const size_t m0 = C.in_group ? (size_t)mid : 0;
  const int M = C.in_group ? rows[mid] : 0, N = C.in_group ? cols[mid] : 0;
  const bool live = C.in_group && M >= 4 && N >= 4;
  // wave-uniform bounds: more than one band only where LP = 64, one matrix per wave
  const int nbands = (int)wave_max_u32(live ? (unsigned)((M + 64 * R - 1) / (64 * R)) : 0u);
  const int S_end = (int)wave_max_u32(live ? (unsigned)(N + LP - 1) : 0u);
  const uint16_t* const Wm = W + m0 * wstride;
  double best = 0.0;  // this lane's maximum so far, its end key and (tracing) the origin of that cell
  uint32_t bkey = 0u, borg = 0u;
  for (int band = 0; band < nbands; ++band) {
    const int row0 = (band * LP + ll) * R;
    const bool rows_ok = live && row0 < M;
    const uint16_t* wr = Wm + (size_t)(row0 >> 4) * ldw;
    const int sh = row0 & 15;
    auto word = [&](int c) -> unsigned {
      return (rows_ok && c >= 0 && c < N) ? (((unsigned)wr[c] >> sh) & kMask) : 0u;
    };
    const SwtRec* const bin = bnd + m0 * bnd_stride + (size_t)(band - 1) * N;
    SwtRec* const bout = bnd + m0 * bnd_stride + (size_t)band * N;
    const bool reads = ll == 0 && band > 0, writes = ll == LP - 1 && band + 1 < nbands;
    uint16_t* const prow = DIR ? plane + m0 * plane_stride + (size_t)(row0 >> 3) * ldp : nullptr;
    // key of (this lane's row 0, column 0) of the walk as a cell of the binary matrix: both minus one
    const uint32_t key0 = ((uint32_t)(row0 - 1) << 16) - 1u;
    double s1[R], s2[R];  // columns c-1, c-2
    uint32_t o1[R], o2[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      s1[r] = s2[r] = 0.0;
      o1[r] = o2[r] = 0u;
    }
    uint32_t w1 = 0, w2 = 0, w3 = 0;  // B bits of my rows at c-1, c-2, c-3
    SwAboveT h1{}, h2{}, h3{};
    SwAboveT pub{};  // what this lane hands down, one step late
    uint32_t q0 = word(-ll), q1 = word(1 - ll), q2 = word(2 - ll), q3 = word(3 - ll);
    for (int s = 0; s < S_end; ++s) {
      const int c = s - ll;
      const uint32_t w0 = q0;
      q0 = q1;
      q1 = q2;
      q2 = q3;
      q3 = word(c + 4);
      const bool incol = c >= 0 && c < N;
      SwAboveT h0;
      h0.sa = __shfl_up(pub.sa, 1);
      h0.sb = __shfl_up(pub.sb, 1);
      h0.b = (uint32_t)__shfl_up((int)pub.b, 1);
      if (!DIR) {
        h0.oa = (uint32_t)__shfl_up((int)pub.oa, 1);
        h0.ob = (uint32_t)__shfl_up((int)pub.ob, 1);
      }
      if (ll == 0) {  // the chain's first lane: the band above, or nothing
        h0 = SwAboveT{};
        if (reads && incol) {
          const SwtRec v = bin[c];
          h0 = SwAboveT{{v.sa, v.sb, v.b}, v.oa, v.ob};
        }
      }
      const uint32_t e1 = (w1 << 3) | h1.b;
      const uint32_t e2 = (w2 << 3) | h2.b;
      const uint32_t e3 = (w3 << 3) | h3.b;
      const bool cok = c >= 3 && c < N;
      const uint32_t kc = key0 + (uint32_t)c;  // key of (row 0, c); only used where the cell scores
      double s0[R];
      uint32_t o0[R];
      double cb = 0.0;  // this column's first maximum, its key and origin
      uint32_t ck = 0u, co = 0u, codes = 0u;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int i = row0 + r;
        const SwCell x = sw_cell<R>(s1, s2, h1, h2, e1, e2, e3, r, cok && i >= 3 && i < M);
        const uint32_t key = kc + ((uint32_t)r << 16);
        uint32_t o = 0u;
        if (DIR) {
          // 0: the cell scores 0, or its chosen predecessor does and the path begins here
          const uint32_t k = (x.v > 0.0 && x.ps > 0.0) ? x.k : 0u;
          codes |= k << (2 * r);
          // Pinned row by row, as crp_dp.hip pins its word: left alone the compiler sinks every
          // code's selects to the store below and carries their compare masks across the row loop.
          asm volatile("" : "+v"(codes));
        } else {
          const uint32_t Oa = r >= 1 ? o1[r - 1] : h1.ob;
          const uint32_t Ob = r >= 2 ? o1[r - 2] : (r == 1 ? h1.ob : h1.oa);
          const uint32_t Oc = r >= 1 ? o2[r - 1] : h2.ob;
          o = x.k == 1u ? Oa : (x.k == 2u ? Ob : Oc);
          o = x.ps > 0.0 ? o : key;  // the chosen predecessor scores 0: the path begins here
          asm volatile("" : "+v"(o));  // beside its score, as crp_dp.hip pins its origins
        }
        if (x.v > cb) {
          cb = x.v;
          ck = key;
          co = o;
        }
        s0[r] = x.v;
        o0[r] = o;
      }
      if (cb > best || (cb == best && cb > 0.0 && ck < bkey)) {
        best = cb;
        bkey = ck;
        borg = co;
      }
      if (DIR) {
        if (rows_ok && incol) prow[c] = (uint16_t)codes;
      }
      pub.sa = s0[R - 2];
      pub.sb = s0[R - 1];
      pub.b = (w0 >> (R - 3)) & 7u;
      pub.oa = o0[R - 2];
      pub.ob = o0[R - 1];
      if (writes && incol) bout[c] = SwtRec{pub.sa, pub.sb, pub.b, pub.oa, pub.ob, 0u};
#pragma unroll
      for (int r = 0; r < R; ++r) {
        s2[r] = s1[r];
        s1[r] = s0[r];
        if (!DIR) {
          o2[r] = o1[r];
          o1[r] = o0[r];
        }
      }
      w3 = w2;
      w2 = w1;
      w1 = w0;
      h3 = h2;
      h2 = h1;
      h1 = h0;
    }
    __threadfence_block();
    __syncthreads();
  }
  // per-chain (score, end key, origin) through LDS, by the per-cell rule (chains need not be a power
  // of two wide)
  s_best[lane] = best;
  s_key[lane] = bkey;
  s_org[lane] = borg;
  __syncthreads();
  if (C.in_group && ll == 0) {
    double m = 0.0;
    uint32_t mk = 0u, mo = 0u;
    for (int t = 0; t < LP; ++t) {
      const double v = s_best[lane + t];
      const uint32_t k = s_key[lane + t];
      if (v > m || (v == m && v > 0.0 && k < mk)) {
        m = v;
        mk = k;
        mo = s_org[lane + t];
      }
    }
    const bool any = live && m > 0.0;
    if (score_out) score_out[mid] = any ? m : 0.0;
    if (DIR) {
      endkey[mid] = any ? mk : kSwNoEnd;
    } else {
      int32_t* sg = seg_out + 4 * (size_t)mid;
      sg[0] = any ? (int)(mo >> 16) : -1;
      sg[1] = any ? (int)(mo & 0xffffu) : -1;
      sg[2] = any ? (int)(mk >> 16) : -1;
      sg[3] = any ? (int)(mk & 0xffffu) : -1;
    }
  }
}

// One wave per matrix. Lane 0 walks the plane from the end cell: note the cell, read its code, step
// to the predecessor, stop at code 0. A counted loop of at most min(sw_path_bound(M, N), path_cap)
// cells that only reads cells in [2, M-2] x [2, N-2] (it ends when a step would leave them), so
// whatever the plane holds it ends, reads inside the matrix's plane and writes inside its path_cap
// entries. Then the whole wave turns the cells round and fills the rest with -1.
__global__ __launch_bounds__(64) void k_sw_backtrack(const uint16_t* __restrict__ plane, int64_t plane_stride, int ldp,
                                                     const int32_t* __restrict__ rows,
                                                     const int32_t* __restrict__ cols,
                                                     const uint32_t* __restrict__ endkey, int path_cap,
                                                     int32_t* __restrict__ seg_out, int32_t* __restrict__ len_out,
                                                     int32_t* path_out) {
  __shared__ int s_n;
  const int mid = blockIdx.x;
  const int lane = threadIdx.x;
  int2* const out = reinterpret_cast<int2*>(path_out) + (size_t)mid * path_cap;
  if (lane == 0) {
    const int M = rows[mid], N = cols[mid];
    const uint32_t key = endkey[mid];
    int r = (int)(key >> 16), c = (int)(key & 0xffffu);
    int n = 0, r0 = -1, c0 = -1, r1 = -1, c1 = -1;
    if (key != kSwNoEnd && r >= 2 && r <= M - 2 && c >= 2 && c <= N - 2) {
      const uint16_t* const pl = plane + (size_t)mid * plane_stride;
      const int lim = min(sw_path_bound(M, N), path_cap);
      r1 = r;
      c1 = c;
      while (n < lim) {
        out[n++] = make_int2(r, c);
        r0 = r;
        c0 = c;
        // cell (r, c) is row r + 1, column c + 1 of the walk
        const uint32_t code = ((uint32_t)pl[(size_t)((r + 1) >> 3) * ldp + (c + 1)] >> (2 * ((r + 1) & 7))) & 3u;
        if (code == 0u) break;
        r -= code == 2u ? 2 : 1;
        c -= code == 3u ? 2 : 1;
        if (r < 2 || c < 2) break;
      }
    }
    if (seg_out) {
      int32_t* sg = seg_out + 4 * (size_t)mid;
      sg[0] = r0;
      sg[1] = c0;
      sg[2] = r1;
      sg[3] = c1;
    }
    len_out[mid] = n;
    s_n = n;
  }
  __threadfence_block();
  __syncthreads();
  path_turn_and_pad(out, s_n, path_cap, lane);
}

// Byte matrices (acoss_sw_constrained's layout) -> bit planes; flags elements other than 0/1.
__global__ void k_sw_pack(const uint8_t* __restrict__ mats, const int64_t* __restrict__ off,
                          const int32_t* __restrict__ rows, const int32_t* __restrict__ cols, uint16_t* __restrict__ W,
                          int64_t wstride, int ldw, int* __restrict__ err) {
  const int mid = blockIdx.x, g = blockIdx.y;
  const int c = blockIdx.z * blockDim.x + threadIdx.x;
  const int M = rows[mid], N = cols[mid];
  if (c >= N || 16 * g >= M) return;
  const uint8_t* B = mats + off[mid];
  unsigned w = 0;
  bool bad = false;
  for (int r = 0; r < 16; ++r) {
    const int i = 16 * g + r;
    if (i < M) {
      const uint8_t v = B[(size_t)i * N + c];
      bad |= v > 1;
      w |= (unsigned)(v != 0) << r;
    }
  }
  W[(size_t)mid * wstride + (size_t)g * ldw + c] = (uint16_t)w;
  if (bad) atomicOr(err, 1);
}

int sw_rows_per_lane(int max_rows) { return max_rows <= 512 ? 8 : 16; }

// lanes per matrix: as many as hold max_rows at 8 rows each while two or more matrices share a
// wave, else the whole wave
int swt_chain(int max_rows) {
  const int LP = (max_rows + kR - 1) / kR;
  return LP < 1 ? 1 : (LP <= 32 ? LP : 64);
}

int64_t swt_bnd_records(int max_rows, int max_cols) {
  const int nbands = (max_rows + 64 * kR - 1) / (64 * kR);
  return nbands > 1 ? (int64_t)nbands * max_cols : 1;
}

template <bool DIR>
void launch_swt(const uint16_t* W, int64_t wstride, int ldw, const int32_t* rows, const int32_t* cols, int n,
                int max_rows, int max_cols, void* bnd, void* plane, double* score, int32_t* seg, uint32_t* endkey,
                hipStream_t s) {
  const int LP = swt_chain(max_rows), G = 64 / LP;
  hipLaunchKernelGGL(k_swt<DIR>, dim3((unsigned)((n + G - 1) / G)), dim3(64), 0, s, W, wstride, ldw, rows, cols, n, LP,
                     static_cast<SwtRec*>(bnd), swt_bnd_records(max_rows, max_cols), static_cast<uint16_t*>(plane),
                     (int64_t)(swt_plane_bytes(max_rows, max_cols) / 2), swt_plane_pitch(max_cols), score, seg, endkey);
}

}  // namespace

size_t sw_bnd_bytes(int max_rows, int max_cols) {
  const int R = sw_rows_per_lane(max_rows);
  const int nbands = (max_rows + 64 * R - 1) / (64 * R);
  return nbands > 1 ? 32 * (size_t)nbands * align_up((size_t)max_cols, 8) : 32;
}

int launch_swb_batch(const uint16_t* W, int64_t wstride, int ldw, const int32_t* rows, const int32_t* cols, int n,
                     int max_rows, int max_cols, void* bnd, double* out, hipStream_t s) {
  const int64_t bstride = (int64_t)(sw_bnd_bytes(max_rows, max_cols) / 32);
  const int LP = (max_rows + 7) / 8;  // lanes per matrix at 8 rows per lane
  if (LP <= 32) {  // two or more matrices per wave (Da-TACOS EarlyFusion: +18 % over one per wave)
    const int G = 64 / LP;
    hipLaunchKernelGGL(k_swb_grp, dim3((unsigned)((n + G - 1) / G)), dim3(64), 0, s, W, wstride, ldw, rows, cols, n, LP,
                       out);
  } else if (sw_rows_per_lane(max_rows) == 8)
    hipLaunchKernelGGL(k_swb<8>, dim3(n), dim3(64), 0, s, W, wstride, ldw, rows, cols, static_cast<double4*>(bnd),
                       bstride, out);
  else
    hipLaunchKernelGGL(k_swb<16>, dim3(n), dim3(64), 0, s, W, wstride, ldw, rows, cols, static_cast<double4*>(bnd),
                       bstride, out);
  ACOSS_LAUNCH_CHECK();
  return ACOSS_OK;
}

size_t swt_bnd_bytes(int max_rows, int max_cols) { return sizeof(SwtRec) * (size_t)swt_bnd_records(max_rows, max_cols); }

size_t swt_plane_bytes(int max_rows, int max_cols) {
  return align_up((size_t)((max_rows + kR - 1) / kR) * swt_plane_pitch(max_cols) * 2, 256);
}

int launch_swt_locate(const uint16_t* W, int64_t wstride, int ldw, const int32_t* rows, const int32_t* cols, int n,
                      int max_rows, int max_cols, void* bnd, double* score, int32_t* seg, hipStream_t s) {
  prof_begin(PH_DP_TRACE, s);
  launch_swt<false>(W, wstride, ldw, rows, cols, n, max_rows, max_cols, bnd, nullptr, score, seg, nullptr, s);
  ACOSS_LAUNCH_CHECK();
  prof_end(PH_DP_TRACE, s);
  return ACOSS_OK;
}

int launch_swt_path(const uint16_t* W, int64_t wstride, int ldw, const int32_t* rows, const int32_t* cols, int n,
                    int max_rows, int max_cols, void* bnd, void* plane, uint32_t* endkey, double* score, int path_cap,
                    int32_t* seg, int32_t* len, int32_t* path, hipStream_t s) {
  prof_begin(PH_DP_DIR, s);
  launch_swt<true>(W, wstride, ldw, rows, cols, n, max_rows, max_cols, bnd, plane, score, nullptr, endkey, s);
  ACOSS_LAUNCH_CHECK();
  prof_end(PH_DP_DIR, s);
  prof_begin(PH_BACKTRACK, s);
  hipLaunchKernelGGL(k_sw_backtrack, dim3(n), dim3(64), 0, s, static_cast<const uint16_t*>(plane),
                     (int64_t)(swt_plane_bytes(max_rows, max_cols) / 2), swt_plane_pitch(max_cols), rows, cols, endkey,
                     path_cap, seg, len, path);
  ACOSS_LAUNCH_CHECK();
  prof_end(PH_BACKTRACK, s);
  return ACOSS_OK;
}

// --------------------------------------------------------------------------------------
// Host entries over byte matrices.
// --------------------------------------------------------------------------------------
namespace {

// The workspace slots of this file (the other files number their own).
enum SwSlot {
  SLOT_SW = 7,         // acoss_sw_constrained
  SLOT_SW_WHERE = 26,  // acoss_sw_locate, acoss_sw_path
};

// A batch of byte matrices as the walks take it, in one workspace slot: the error flag at 0, then
// from 256 the band-boundary records, the bit planes and, for the path entry alone, the direction
// planes and the end keys, each region aligned to 256 B.
struct SwBatch {
  int* d_err;
  void* bnd;
  uint16_t* W;
  int64_t wstride;
  int ldw;
  void* plane;
  uint32_t* endkey;
};

// Lays the slot out and packs the matrices into bit planes (k_sw_pack raises the error flag at an
// element above 1) on stream s. bnd_bytes, plane_bytes: per matrix; end keys (4 bytes per matrix)
// come with the planes.
int sw_pack(int slot, const uint8_t* mats, const int64_t* off, const int32_t* rows, const int32_t* cols, int n_mats,
            int max_rows, int max_cols, size_t bnd_bytes, size_t plane_bytes, hipStream_t s, SwBatch& B) {
  const int G = (max_rows + 15) / 16;
  const int ldw = (int)align_up((size_t)max_cols, 4);
  const int64_t wstride = (int64_t)G * ldw;
  const size_t bnd_b = align_up(bnd_bytes * n_mats, 256);
  const size_t w_b = align_up((size_t)wstride * 2 * n_mats, 256);
  const size_t plane_b = plane_bytes * n_mats;
  const size_t key_b = plane_bytes ? 4 * (size_t)n_mats : 0;
  char* ws = static_cast<char*>(workspace(slot, 256 + bnd_b + w_b + plane_b + key_b));
  if (!ws) return ACOSS_E_HIP;
  B = SwBatch{reinterpret_cast<int*>(ws),
              ws + 256,
              reinterpret_cast<uint16_t*>(ws + 256 + bnd_b),
              wstride,
              ldw,
              ws + 256 + bnd_b + w_b,
              reinterpret_cast<uint32_t*>(ws + 256 + bnd_b + w_b + plane_b)};
  ACOSS_HIP_CHECK(hipMemsetAsync(B.d_err, 0, 4, s));
  if (G > 0 && max_cols > 0) {
    hipLaunchKernelGGL(k_sw_pack, dim3(n_mats, G, (max_cols + 255) / 256), dim3(256), 0, s, mats, off, rows, cols, B.W,
                       wstride, ldw, B.d_err);
    ACOSS_LAUNCH_CHECK();
  }
  return ACOSS_OK;
}

// After the entry's launches: waits for them and refuses a batch that k_sw_pack flagged.
int sw_finish(const SwBatch& B, hipStream_t s) {
  int h_err = 0;
  ACOSS_HIP_CHECK(hipMemcpyAsync(&h_err, B.d_err, 4, hipMemcpyDeviceToHost, s));
  ACOSS_HIP_CHECK(hipStreamSynchronize(s));
  if (h_err) {
    set_error("smith_waterman_constrained: Non-binary elements found in input");
    return ACOSS_E_NONBINARY;
  }
  return ACOSS_OK;
}

// acoss_sw_locate (path = false) and acoss_sw_path: acoss_sw_constrained's packing, then the
// tracing DP, or the direction DP and the walk back.
int sw_where(const char* entry, bool path, const uint8_t* mats, const int64_t* off, const int32_t* rows,
             const int32_t* cols, int32_t n_mats, int32_t max_rows, int32_t max_cols, double* score_out,
             int32_t* seg_out, int32_t path_cap, int32_t* len_out, int32_t* path_out, void* hip_stream) {
  clear_error();
  if (n_mats < 0 || max_rows < 0 || max_cols < 0 ||
      (n_mats > 0 && (!mats || !off || !rows || !cols || (path ? !len_out || !path_out : !seg_out)))) {
    set_error("%s: bad arguments", entry);
    return ACOSS_E_ARG;
  }
  if (max_rows > kSwCellMax || max_cols > kSwCellMax) {
    set_error("%s: %d x %d: a cell is packed into 16 + 16 bits, at most %d rows and columns", entry, max_rows,
              max_cols, kSwCellMax);
    return ACOSS_E_SHAPE;
  }
  const int bound = std::max(1, sw_path_bound(max_rows, max_cols));
  if (path && path_cap < bound) {
    set_error("%s: path_cap %d below max(1, min(max_rows, max_cols) - 3) = %d: a path may have that many cells", entry,
              path_cap, bound);
    return ACOSS_E_ARG;
  }
  if (n_mats == 0) return ACOSS_OK;
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  SwBatch B;
  int rc = sw_pack(SLOT_SW_WHERE, mats, off, rows, cols, n_mats, max_rows, max_cols,
                   swt_bnd_bytes(max_rows, max_cols), path ? swt_plane_bytes(max_rows, max_cols) : 0, s, B);
  if (rc) return rc;
  rc = path ? launch_swt_path(B.W, B.wstride, B.ldw, rows, cols, n_mats, max_rows, max_cols, B.bnd, B.plane, B.endkey,
                              score_out, path_cap, seg_out, len_out, path_out, s)
            : launch_swt_locate(B.W, B.wstride, B.ldw, rows, cols, n_mats, max_rows, max_cols, B.bnd, score_out,
                                seg_out, s);
  if (rc) return rc;
  return sw_finish(B, s);
}

}  // namespace

}  // namespace acoss

using namespace acoss;

extern "C" int acoss_sw_constrained(const uint8_t* mats, const int64_t* off, const int32_t* rows, const int32_t* cols,
                                    int32_t n_mats, int32_t max_rows, int32_t max_cols, double* score_out,
                                    void* hip_stream) {
  clear_error();
  if (n_mats < 0 || (n_mats > 0 && (!mats || !off || !rows || !cols || !score_out)) || max_rows < 0 || max_cols < 0) {
    set_error("acoss_sw_constrained: bad arguments");
    return ACOSS_E_ARG;
  }
  if (n_mats == 0) return ACOSS_OK;
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  prof_begin(PH_SW, s);
  SwBatch B;
  int rc = sw_pack(SLOT_SW, mats, off, rows, cols, n_mats, max_rows, max_cols, sw_bnd_bytes(max_rows, max_cols), 0, s, B);
  if (rc) return rc;
  rc = launch_swb_batch(B.W, B.wstride, B.ldw, rows, cols, n_mats, max_rows, max_cols, B.bnd, score_out, s);
  if (rc) return rc;
  prof_end(PH_SW, s);
  return sw_finish(B, s);
}

extern "C" int acoss_sw_locate(const uint8_t* mats, const int64_t* off, const int32_t* rows, const int32_t* cols,
                               int32_t n_mats, int32_t max_rows, int32_t max_cols, double* score_out,
                               int32_t* seg_out, void* hip_stream) {
  return sw_where("acoss_sw_locate", false, mats, off, rows, cols, n_mats, max_rows, max_cols, score_out, seg_out, 0,
                  nullptr, nullptr, hip_stream);
}

extern "C" int acoss_sw_path(const uint8_t* mats, const int64_t* off, const int32_t* rows, const int32_t* cols,
                             int32_t n_mats, int32_t max_rows, int32_t max_cols, double* score_out, int32_t* seg_out,
                             int32_t path_cap, int32_t* len_out, int32_t* path_out, void* hip_stream) {
  return sw_where("acoss_sw_path", true, mats, off, rows, cols, n_mats, max_rows, max_cols, score_out, seg_out,
                  path_cap, len_out, path_out, hip_stream);
}
