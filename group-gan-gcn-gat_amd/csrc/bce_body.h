// The value of the adversarial loss (loss.hip: sgg_bce_fwd), shared by its
// stand-alone kernel and by the loss workgroup of the weight-gradient finish
// launch (grad.hip: sgg_grad_finish_losses, SggBceJob).  Both run it with
// kBceThreads threads, so every sum has ONE order -- thread t adds the scores
// t, t + kBceThreads, ... of each range in index order, a wave shuffle tree,
// then the waves' sums in wave order -- and both users produce the same bits.
#pragma once
#include "sgg_common.h"

namespace sgg {

constexpr int kBceThreads = 1024;   // the workgroup of both users
constexpr int kBcePre = 8;          // scores per thread loaded ahead (8,192: one round trip)

//   f(x, y) = max(x, 0) - x y + log(1 + exp(-|x|))   (losses.py:5-21)
__device__ __forceinline__ float bce_term(float x, float y) {
  return fmaxf(x, 0.f) - x * y + logf(1.f + expf(-fabsf(x)));
}

// the score i counts: inside its range's first nv scores
__device__ __forceinline__ bool bce_live(int i, int split, int nv) { return i < split ? i < nv : i - split < nv; }

// a job's inputs, loaded before anything waits (one round trip for all)
struct BceIn {
  float v[kBcePre], a, b;
  int nv;
};
__device__ __forceinline__ void bce_load(const SggBceJob& d, BceIn& in) {
  in.a = *d.ya;
  in.b = *d.yb;
  in.nv = d.nvalid ? *d.nvalid : d.n;
#pragma unroll
  for (int m = 0; m < kBcePre; ++m) {
    const int i = threadIdx.x + kBceThreads * m;
    in.v[m] = i < d.n ? d.x[i] : 0.f;
  }
}

// *loss = w (mean_{i < split} f(x_i, ya) + mean_{i >= split} f(x_i, yb)) over
// the first nvalid scores of each range; *total = *loss + addend when total !=
// NULL.  red: 2 x (kBceThreads / 64) floats of LDS; every thread of the
// workgroup calls it (two workgroup barriers).
__device__ __forceinline__ void bce_value(const SggBceJob& d, const BceIn& in, float addend,
                                          float (*red)[kBceThreads / 64]) {
  float s0 = 0.f, s1 = 0.f;
#pragma unroll
  for (int m = 0; m < kBcePre; ++m) {
    const int i = threadIdx.x + kBceThreads * m;
    if (i < d.n && bce_live(i, d.split, in.nv)) {
      if (i < d.split) s0 += bce_term(in.v[m], in.a);
      else s1 += bce_term(in.v[m], in.b);
    }
  }
  for (int i = threadIdx.x + kBcePre * kBceThreads; i < d.n; i += kBceThreads) {   // past the prefetched scores
    if (bce_live(i, d.split, in.nv)) {
      if (i < d.split) s0 += bce_term(d.x[i], in.a);
      else s1 += bce_term(d.x[i], in.b);
    }
  }
  s0 = wave_sum(s0);
  s1 = wave_sum(s1);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    red[0][wave] = s0;
    red[1][wave] = s1;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float t0 = 0.f, t1 = 0.f;
#pragma unroll
    for (int w = 0; w < kBceThreads / 64; ++w) {
      t0 += red[0][w];
      t1 += red[1][w];
    }
    const int c0 = min(d.split, in.nv), c1 = min(d.n - d.split, in.nv);
    const float m0 = c0 > 0 ? t0 / (float)c0 : 0.f;
    const float m1 = c1 > 0 ? t1 / (float)c1 : 0.f;
    const float l = d.w * (m0 + m1);
    *d.loss = l;
    if (d.total) *d.total = l + addend;
  }
  __syncthreads();
}

}  // namespace sgg
