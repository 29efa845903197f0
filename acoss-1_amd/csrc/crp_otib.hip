// crp_otib.hip — the OTI-binary CRP (Serra08), the second mask producer under the Serra09 / Chen
// aligners (the definition: include/acoss_hip.h, acoss_crp_params2).
//
// A cell (i, j) is a hit when fewer than oti_rank of the eleven further transpositions of the
// reference's stacked frame j lie strictly closer to the query's stacked frame i than the
// transposition the pair's global OTI already applied. No percentile, so no order statistics: the
// cost is twelve Grams and twelve windows per cell where the percentile CRP builds one.
//
// k_crp_otib<COUNT>: one 256-thread block per (pair, strip of 32 query rows, panel of 256 reference
// columns), the shape of crp.hip's k_crp_panel. The query frames (Xs) and the UN-rolled reference
// frames (Ys) are staged in LDS once; then, per shift k = 0 .. 11, the Gram of the panel with the
// reference bins rolled by (g + k) mod 12 goes to LDS (Gs) as fmaf chains in bin order, and each
// thread (one column) adds the m window taps of its 32 cells in tap order and forms the key
// max((N_query - 2 dot) + N_reference, +0): the float32 squared distance acoss_crp_pair's dist is the
// sqrt_rn of, bit for bit. The 32 keys of shift 0 stay in registers; against them a thread holds a
// 32-bit mask of the rows no shift has beaten yet (COUNT = false, oti_rank = 1) or 32 four-bit
// counts of the shifts that did (COUNT = true). Staging, norms, the launch and the un-rolled
// operands are shared by the twelve shifts; the roll is an index into Ys when a thread loads its
// column's twelve bins.
//
// The Gram pass is balanced: thread t owns column t of the panel for all GR rows (its twelve y in
// registers, the x rows broadcast from LDS); the m - 1 halo columns 256 .. GW - 1 are dealt out
// cell by cell over the whole block instead of being a second pass of wave 0.
//
// sqrt only where two keys are close. The definition compares D = sqrt_rn(key). For float32
// 0 <= a < b:
//   (1) sqrt_rn is monotone, so a >= b gives sqrt_rn(a) >= sqrt_rn(b): not closer, no root needed.
//   (2) if b >= a (1 + 2^-21) then sqrt_rn(a) < sqrt_rn(b). Proof: sqrt(b) / sqrt(a) >=
//       sqrt(1 + 2^-21) > 1 + 2^-22 - 2^-44, so with 2^e <= sqrt(a) < 2^(e+1) and h = 2^(e-23), the
//       spacing of the floats of that binade, sqrt(b) - sqrt(a) > 2^e (2^-22 - 2^-44) =
//       2 h (1 - 2^-22) > 1.5 h. Two reals x < y of one binade with y - x > h round to different
//       floats (rn(x) <= x + h/2 < y - h/2 <= rn(y)); if y lies in the next binade (spacing 2 h) both
//       can round to 2^(e+1) only when x >= 2^(e+1) - h/2 and y <= 2^(e+1) + h, i.e. y - x <= 1.5 h.
//       Either way the rounded roots differ, and by (1) in the right order.
//   (3) the kernel's test a <= lo with lo = fl(b (1 - 2^-20)), taken only for b >= 2^-100 (so the
//       product is a normal number and fl's relative error is at most 2^-24), implies (2):
//       lo < b (1 - 2^-20)(1 + 2^-24) < b (1 - 15/16 2^-20), hence b > a (1 + 15/16 2^-20) > a (1 + 2^-21).
//       Below 2^-100 lo is -1 and no key passes.
// Keys with lo < a < b (a relative gap under 2^-20: ties in all but the last bits) take both roots.
#include "crp_internal.hpp"

namespace acoss {

namespace {

constexpr int kOtibW = 256;  // columns per panel = threads per block
constexpr int kOtibR = 32;   // rows per panel = one strip of mask words

__host__ __device__ inline size_t otib_lds_floats(int m) {
  const int GR = kOtibR + m - 1, GW = kOtibW + m - 1;
  return align_up((size_t)GR * 12, 4) + align_up((size_t)GW * 13, 4) + (size_t)GR * GW;
}

// One Gram entry: the fmaf chain over the 12 bins in bin order, x a row of Xs, y the rolled bins.
__device__ __forceinline__ float gram12(const float* __restrict__ x, const float (&y)[12]) {
  const float4* xr = reinterpret_cast<const float4*>(x);
  const float4 x0 = xr[0], x1 = xr[1], x2 = xr[2];
  float acc = 0.0f;
  acc = __builtin_fmaf(x0.x, y[0], acc);
  acc = __builtin_fmaf(x0.y, y[1], acc);
  acc = __builtin_fmaf(x0.z, y[2], acc);
  acc = __builtin_fmaf(x0.w, y[3], acc);
  acc = __builtin_fmaf(x1.x, y[4], acc);
  acc = __builtin_fmaf(x1.y, y[5], acc);
  acc = __builtin_fmaf(x1.z, y[6], acc);
  acc = __builtin_fmaf(x1.w, y[7], acc);
  acc = __builtin_fmaf(x2.x, y[8], acc);
  acc = __builtin_fmaf(x2.y, y[9], acc);
  acc = __builtin_fmaf(x2.z, y[10], acc);
  acc = __builtin_fmaf(x2.w, y[11], acc);
  return acc;
}

// Bins of reference frame b of the panel as np.roll(frame, roll) has them: y[c] = frame[(c - roll) mod 12].
__device__ __forceinline__ void rolled_bins(const float* __restrict__ Ys, int b, int roll, float (&y)[12]) {
  const float* f = Ys + b * 13;
  int src = roll == 0 ? 0 : 12 - roll;  // (0 - roll) mod 12
#pragma unroll
  for (int c = 0; c < 12; ++c) {
    y[c] = f[src];
    src = src == 11 ? 0 : src + 1;
  }
}

template <bool COUNT>
__global__ __launch_bounds__(256) void k_crp_otib(CrpBatch B, int oti_rank, uint32_t* __restrict__ maskT,
                                                  int64_t mask_stride, int ld, uint8_t* __restrict__ closer) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int R = kOtibR;
  const int p = blockIdx.z;
  const int2 dm = B.dims[p];
  const int strip = blockIdx.y;
  const int i0 = strip * R, j0 = blockIdx.x * kOtibW;
  if (i0 >= dm.x || j0 >= dm.y) return;
  const int ta = B.pairs[2 * p], tb = B.pairs[2 * p + 1];
  const int g = B.oti[p];
  const int m = B.m, tau = B.tau, GR = R + m - 1, GW = kOtibW + m - 1;
  float* Xs = smem;
  float* Ys = Xs + align_up((size_t)GR * 12, 4);
  float* Gs = Ys + align_up((size_t)GW * 13, 4);
  const float* xq = B.feats + B.off[ta] * 12;
  const float* yr = B.feats + B.off[tb] * 12;
  const int nq = B.len[ta], nr = B.len[tb];
  // staged once for the twelve shifts: query rows and un-rolled reference columns, 0 past the track
  for (int e = threadIdx.x; e < GR * 12; e += blockDim.x) {
    const int a = e / 12, c = e - a * 12;
    const int f = (i0 + a) * tau;
    Xs[e] = f < nq ? xq[(size_t)f * 12 + c] : 0.0f;
  }
  for (int e = threadIdx.x; e < GW * 12; e += blockDim.x) {
    const int b = e / 12, c = e - b * 12;
    const int f = (j0 + b) * tau;
    Ys[b * 13 + c] = f < nr ? yr[(size_t)f * 12 + c] : 0.0f;
  }
  const int t = threadIdx.x, j = j0 + t;
  const bool live = j < dm.y;
  const int rows = min(R, dm.x - i0);
  const float* NXq = B.NX + (size_t)ta * B.ldn + i0;
  const float nin = live ? B.NX[(size_t)tb * B.ldn + j] : 0.0f;
  float key0[R], lo[R];
  uint32_t alive = rows == R ? 0xffffffffu : ((1u << rows) - 1u);  // COUNT = false: rows no shift has beaten
  uint32_t cnt[4] = {0u, 0u, 0u, 0u};                               // COUNT = true: 4 bits per row
  const int halo = (m - 1) * GR;  // Gram entries of the columns 256 .. GW - 1
  __syncthreads();
#pragma unroll 1
  for (int k = 0; k < 12; ++k) {
    int roll = g + k;
    roll = roll >= 12 ? roll - 12 : roll;
    {
      float y[12];
      rolled_bins(Ys, t, roll, y);
      for (int a = 0; a < GR; ++a) Gs[a * GW + t] = gram12(Xs + a * 12, y);
      for (int e = t; e < halo; e += kOtibW) {
        const int a = e / (m - 1), b = kOtibW + (e - a * (m - 1));
        rolled_bins(Ys, b, roll, y);
        Gs[a * GW + b] = gram12(Xs + a * 12, y);
      }
    }
    __syncthreads();
    if (live) {
#pragma unroll
      for (int r = 0; r < R; ++r) {
        if (r < rows) {
          float dot = 0.0f;
          for (int u = 0; u < m; ++u) dot = dot + Gs[(r + u) * GW + t + u];
          const float d2 = (NXq[r] - 2.0f * dot) + nin;  // canonical: (N_query - 2 dot) + N_reference
          const float a = d2 > 0.0f ? d2 : 0.0f;
          if (k == 0) {
            key0[r] = a;
            lo[r] = a >= 0x1p-100f ? a * (1.0f - 0x1p-20f) : -1.0f;
          } else {
            bool nearer = a <= lo[r];
            if (a > lo[r] && a < key0[r]) nearer = sqrt_rn(a) < sqrt_rn(key0[r]);
            if (COUNT)
              cnt[r >> 3] += (uint32_t)nearer << (4 * (r & 7));
            else
              alive &= ~((uint32_t)nearer << r);
          }
        }
      }
    }
    __syncthreads();
  }
  if (!live) return;
  uint32_t bits = alive;
  if (COUNT) {
    bits = 0u;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if (r < rows) {
        const uint32_t c = (cnt[r >> 3] >> (4 * (r & 7))) & 15u;
        bits |= (uint32_t)(c < (uint32_t)oti_rank) << r;
        if (closer) closer[(size_t)(i0 + r) * dm.y + j] = (uint8_t)c;
      }
    }
  }
  maskT[(size_t)p * mask_stride + (size_t)strip * ld + j] = bits;
}

}  // namespace

int launch_otib(const CrpBatch& B, int nb, int L, int oti_rank, uint32_t* maskT, int64_t mask_stride, int ld,
                hipStream_t s, uint8_t* closer) {
  const size_t lds = otib_lds_floats(B.m) * sizeof(float);
  const bool count = oti_rank > 1 || closer;
  const void* kernel = count ? reinterpret_cast<const void*>(k_crp_otib<true>)
                             : reinterpret_cast<const void*>(k_crp_otib<false>);
  if (lds > 64 * 1024)
    ACOSS_HIP_CHECK(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  const dim3 grid((L + kOtibW - 1) / kOtibW, (L + kOtibR - 1) / kOtibR, nb);
  if (count)
    hipLaunchKernelGGL(k_crp_otib<true>, grid, dim3(256), lds, s, B, oti_rank, maskT, mask_stride, ld, closer);
  else
    hipLaunchKernelGGL(k_crp_otib<false>, grid, dim3(256), lds, s, B, oti_rank, maskT, mask_stride, ld, closer);
  ACOSS_LAUNCH_CHECK();
  return ACOSS_OK;
}

}  // namespace acoss
