// The operand fetch and K walk of the dense transform Y = X W on fp32 MFMA
// (xw.hip: lane maps and the scheme), and the split-K walk of one 16-row x
// 64-col tile, as device bodies: xw.hip's kernels, and the LSTM backward's
// prologue that forms the pooling backward's dh = dU W1h where it is consumed
// (lstm_mw.hip).
#pragma once
#include "sgg_common.h"

namespace sgg {

constexpr int kXwKC = 16;            // K chunk: 4 MFMA k-steps, double-buffered in registers
constexpr int kXwS4 = kXwKC / 4;
constexpr int kXwStageMaxK = 256;    // TRANS_W weights staged in LDS up to this K

// Operand fetch of one 16-row x 64-col wave tile over k in [kb, kend):
// X rows from global, W from global (row-major K x N, or N x K if TRANS_W)
// or from the LDS image `ws` (64 rows x K at pitch K + 1, TRANS_W staged).
// Loads use clamped (in-bounds) addresses; only k >= kend must contribute
// zero, which concerns the last chunk alone -- a wave-uniform branch (a
// per-load `cond ? v : 0` makes the compiler sink each load into an
// exec-masked branch that waits for it).
template <bool TRANS_W, bool STAGED>
struct XwFrag {
  const float* xrow;
  const float* mrow;
  const float* W;
  const float* ws;
  int ldw, kp, kend;
  int ncl[4];   // clamped global output columns (unstaged) / local rows of ws (staged)
  int kq;

  __device__ __forceinline__ float wval(int t, int k) const {
    if (STAGED) return ws[ncl[t] * kp + k];
    return TRANS_W ? W[(size_t)ncl[t] * ldw + k] : W[(size_t)k * ldw + ncl[t]];
  }
  // k order within a 16-deep chunk is permuted: k-step s of lane quarter kq
  // takes k = kb + 4 kq + s (the same for both operands), so a lane's four
  // A values of a chunk are one 16-byte load (full 64-byte lines per wave
  // instruction instead of 16-byte pieces of 16 lines)
  bool vec;   // X (and the mask) rows 16-byte aligned
  __device__ __forceinline__ void load_a(int kb, float (&aa)[kXwS4]) const {
    if (kb + kXwKC <= kend) {
      if (vec) {
        const float4 v = *reinterpret_cast<const float4*>(xrow + kb + 4 * kq);
        aa[0] = v.x;
        aa[1] = v.y;
        aa[2] = v.z;
        aa[3] = v.w;
        if (mrow) {
          const float4 mv = *reinterpret_cast<const float4*>(mrow + kb + 4 * kq);
          aa[0] = keep_if(aa[0], mv.x > 0.f);
          aa[1] = keep_if(aa[1], mv.y > 0.f);
          aa[2] = keep_if(aa[2], mv.z > 0.f);
          aa[3] = keep_if(aa[3], mv.w > 0.f);
        }
        return;
      }
#pragma unroll
      for (int s = 0; s < kXwS4; ++s) {
        const int k = kb + 4 * kq + s;
        aa[s] = mrow ? keep_if(xrow[k], mrow[k] > 0.f) : xrow[k];
      }
    } else {
#pragma unroll
      for (int s = 0; s < kXwS4; ++s) {
        const int k = kb + 4 * kq + s;
        const int kc = min(k, kend - 1);
        aa[s] = keep_if(xrow[kc], k < kend && (!mrow || mrow[kc] > 0.f));
      }
    }
  }
  __device__ __forceinline__ void load_b(int kb, float (&bb)[kXwS4][4]) const {
#pragma unroll
    for (int s = 0; s < kXwS4; ++s) {
      const int kc = min(kb + 4 * kq + s, kend - 1);   // past kend the A operand is zero
#pragma unroll
      for (int t = 0; t < 4; ++t) bb[s][t] = wval(t, kc);
    }
  }
  __device__ __forceinline__ void load(int kb, float (&aa)[kXwS4], float (&bb)[kXwS4][4]) const {
    load_a(kb, aa);
    load_b(kb, bb);
  }
};

// acc[t] += X[rows, kb0..kend) W[kb0..kend), cols]: the next chunk's loads are
// in flight while the current chunk runs through the MFMAs
// apre: the first chunk's A fragments, already loaded by the caller (issued
// before the weight staging, so the two memory latencies overlap)
template <bool TRANS_W, bool STAGED>
__device__ __forceinline__ void xw_walk(const XwFrag<TRANS_W, STAGED>& f, int kb0, floatx4 (&acc)[4],
                                        const float (*apre)[kXwS4] = nullptr) {
  if (kb0 >= f.kend) return;
  float a0[kXwS4], b0[kXwS4][4], a1[kXwS4], b1[kXwS4][4];
  if (apre) {
#pragma unroll
    for (int s = 0; s < kXwS4; ++s) a0[s] = (*apre)[s];
    f.load_b(kb0, b0);
  } else {
    f.load(kb0, a0, b0);
  }
  for (int k0 = kb0; k0 < f.kend; k0 += 2 * kXwKC) {
    if (k0 + kXwKC < f.kend) f.load(k0 + kXwKC, a1, b1);
#pragma unroll
    for (int s = 0; s < kXwS4; ++s)
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[s], b0[s][t], acc[t], 0, 0, 0);
    if (k0 + kXwKC >= f.kend) break;
    if (k0 + 2 * kXwKC < f.kend) f.load(k0 + 2 * kXwKC, a0, b0);
#pragma unroll
    for (int s = 0; s < kXwS4; ++s)
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[s], b1[s][t], acc[t], 0, 0, 0);
  }
}

constexpr int kXwSplitLds = 4 * 16 * 65;   // LDS floats of one split-K workgroup

// Split-K partial of the 16 x 64 tile at (row0, col0): wave `wave` (0..3)
// walks its quarter of K and leaves its tile in part[wave].  The tile is the
// sum of the four in wave order (xw_splitk_sum), once a barrier has passed.
template <bool TRANS_W>
__device__ __forceinline__ void xw_splitk_walk(const float* __restrict__ X, int ldx, const float* __restrict__ Xmask,
                                               int ldm, const float* __restrict__ W, int ldw, int M, int K, int N,
                                               int row0, int col0, int wave, float (*part)[16][65]) {
  const int lane = threadIdx.x & 63;
  const int ar = lane & 15, kq = lane >> 4;
  const int arow = row0 + ar;
  const bool arow_ok = arow < M;
  const int span = (((K + 3) / 4) + kXwKC - 1) / kXwKC * kXwKC;   // this wave's K range
  XwFrag<TRANS_W, false> f;
  f.xrow = X + (size_t)(arow_ok ? arow : 0) * ldx;
  f.mrow = Xmask ? Xmask + (size_t)(arow_ok ? arow : 0) * ldm : nullptr;
  f.W = W;
  f.ws = nullptr;
  f.ldw = ldw;
  f.kp = 0;
  f.kend = min(K, (wave + 1) * span);
  f.kq = kq;
  f.vec = ((reinterpret_cast<uintptr_t>(X) | (uintptr_t)ldx * 4 |
            (Xmask ? (reinterpret_cast<uintptr_t>(Xmask) | (uintptr_t)ldm * 4) : 0)) & 15) == 0;
#pragma unroll
  for (int t = 0; t < 4; ++t) f.ncl[t] = min(col0 + 16 * t + ar, N - 1);
  floatx4 acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = floatx4{0.f, 0.f, 0.f, 0.f};
  xw_walk(f, wave * span, acc);
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) part[wave][kq * 4 + r][16 * t + ar] = acc[t][r];
}

__device__ __forceinline__ float xw_splitk_sum(const float (*part)[16][65], int rr, int cc) {
  return ((part[0][rr][cc] + part[1][rr][cc]) + part[2][rr][cc]) + part[3][rr][cc];
}

}  // namespace sgg
