// sw_path.hip — where the constrained Smith-Waterman alignment lies: misc.hip's float64 walk
// (k_swb / k_swb_grp) with what a traceback needs carried along, for acoss_sw_locate / acoss_sw_path
// and the four matrices of acoss_earlyfusion_locate / acoss_earlyfusion_path. The definition is in
// include/acoss_hip.h (acoss_sw_locate); tests/sw_path_np.py restates it in numpy.
//
//  k_swt<false>   the tracing DP: beside every S the packed cell (r0 << 16) | c0 where its path began
//  k_swt<true>    the direction DP: a 2-bit predecessor code per cell, written to a plane
//  k_sw_backtrack the walk back over that plane
//
// One kernel body serves every shape launch_swb_batch serves. A chain of LP lanes holds a matrix,
// 8 rows per lane, and sweeps the columns skewed by one per lane as k_swb does:
//  * LP <= 32 (matrices of at most 256 rows): G = 64 / LP matrices per wave, one band each, as
//    k_swb_grp lays them out;
//  * LP = 64: one matrix per wave in bands of 512 rows. The last lane's two rows of scores, three
//    rows of bits and two origins go to the next band through one 32-byte record per column.
// The cell recurrence is k_swb's, operation for operation, so the scores are its scores bit for bit.
// Cells are named in the binary matrix's own coordinates: the walk's row i and column c (those of
// the reference's score matrix) are the cell (i - 1, c - 1).
#include "sw_internal.hpp"

namespace acoss {

namespace {

constexpr int kR = 8;  // rows per lane
constexpr uint32_t kSwNoEnd = 0xffffffffu;

struct SwtAbove {      // what the lane above hands down for one column
  double sa, sb;       // S of its rows R-2, R-1
  uint32_t b;          // B bits of its rows R-3, R-2, R-1 (bits 0..2)
  uint32_t oa, ob;     // origins of the same two cells (tracing DP only)
};

struct SwtRec {  // one column of a band boundary
  double sa, sb;
  uint32_t b, oa, ob, unused;
};
static_assert(sizeof(SwtRec) == 32, "swt_bnd_bytes counts 32-byte records");

// plane of a matrix: row groups of 8 rows of the walk (row i in group i >> 3, bits 2 (i & 7) and
// the next), ldp 16-bit words each, one per column of the walk
__host__ __device__ inline int swt_plane_pitch(int max_cols) { return (int)align_up((size_t)max_cols, 4); }

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
  const int G = 64 / LP;
  const int g = lane / LP, ll = lane - g * LP;
  const int mid = blockIdx.x * G + g;
  const bool in_group = g < G && mid < n;
  const size_t m0 = in_group ? (size_t)mid : 0;
  const int M = in_group ? rows[mid] : 0, N = in_group ? cols[mid] : 0;
  const bool live = in_group && M >= 4 && N >= 4;
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
    unsigned w1 = 0, w2 = 0, w3 = 0;  // B bits of my rows at c-1, c-2, c-3
    SwtAbove h1{0, 0, 0, 0, 0}, h2{0, 0, 0, 0, 0}, h3{0, 0, 0, 0, 0};
    SwtAbove pub{0, 0, 0, 0, 0};  // what this lane hands down, one step late
    unsigned q0 = word(-ll), q1 = word(1 - ll), q2 = word(2 - ll), q3 = word(3 - ll);
    for (int s = 0; s < S_end; ++s) {
      const int c = s - ll;
      const unsigned w0 = q0;
      q0 = q1;
      q1 = q2;
      q2 = q3;
      q3 = word(c + 4);
      const bool incol = c >= 0 && c < N;
      SwtAbove h0;
      h0.sa = __shfl_up(pub.sa, 1);
      h0.sb = __shfl_up(pub.sb, 1);
      h0.b = (unsigned)__shfl_up((int)pub.b, 1);
      if (!DIR) {
        h0.oa = (uint32_t)__shfl_up((int)pub.oa, 1);
        h0.ob = (uint32_t)__shfl_up((int)pub.ob, 1);
      }
      if (ll == 0) {  // the chain's first lane: the band above, or nothing
        h0 = SwtAbove{0, 0, 0, 0, 0};
        if (reads && incol) {
          const SwtRec v = bin[c];
          h0 = SwtAbove{v.sa, v.sb, v.b, v.oa, v.ob};
        }
      }
      // extended bit words: bit r+3 <-> my row r; bits 0..2 <-> rows -3..-1
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
        // the first of a, b, c that attains the maximum, and what that predecessor scores
        double v = x1, ps = A;
        uint32_t k = 1u;
        if (x2 > v) {
          v = x2;
          ps = Bv;
          k = 2u;
        }
        if (x3 > v) {
          v = x3;
          ps = Cv;
          k = 3u;
        }
        v = 0.0 > v ? 0.0 : v;
        const int i = row0 + r;
        v = (cok && i >= 3 && i < M) ? v : 0.0;
        const uint32_t key = kc + ((uint32_t)r << 16);
        uint32_t o = 0u;
        if (DIR) {
          // 0: the cell scores 0, or its chosen predecessor does and the path begins here
          k = (v > 0.0 && ps > 0.0) ? k : 0u;
          codes |= k << (2 * r);
          // Pinned row by row, as crp_dp.hip pins its word: left alone the compiler sinks every
          // code's selects to the store below and carries their compare masks across the row loop.
          asm volatile("" : "+v"(codes));
        } else {
          const uint32_t Oa = r >= 1 ? o1[r - 1] : h1.ob;
          const uint32_t Ob = r >= 2 ? o1[r - 2] : (r == 1 ? h1.ob : h1.oa);
          const uint32_t Oc = r >= 1 ? o2[r - 1] : h2.ob;
          o = k == 1u ? Oa : (k == 2u ? Ob : Oc);
          o = ps > 0.0 ? o : key;  // the chosen predecessor scores 0: the path begins here
          asm volatile("" : "+v"(o));  // beside its score, as crp_dp.hip pins its origins
        }
        if (v > cb) {
          cb = v;
          ck = key;
          co = o;
        }
        s0[r] = v;
        o0[r] = o;
      }
      // The skewed walk does not visit cells in row-major order: among equal scores the smaller key.
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
  if (in_group && ll == 0) {
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

}  // namespace acoss
