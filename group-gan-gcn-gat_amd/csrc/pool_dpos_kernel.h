// The positions' gradient kernel of dec_step.hip, included twice (no include
// guard): with SGG_POOL_DROP 0 this text is pool_dpos_kernel, with SGG_POOL_DROP 1
// pool_dpos_drop_kernel (sgg_pool_dpos_drop), which takes the dropout arguments
// (DropArgs) as one more parameter: g = dout * scale where out > 0, and the hidden
// unit k of the pair (i, j*) carries the hidden mask's factor m1(i, j* - scene
// start, k) of pool_drop.h.  One text so that pool_dpos_kernel keeps its
// instruction stream (as csrc/gat_kernels.h).
#undef SGG_POOL_DPOS_KERNEL
#undef SGG_POOL_DROP_PARAM
#if SGG_POOL_DROP
#define SGG_POOL_DPOS_KERNEL pool_dpos_drop_kernel
#define SGG_POOL_DROP_PARAM , const DropArgs drop
#else
#define SGG_POOL_DPOS_KERNEL pool_dpos_kernel
#define SGG_POOL_DROP_PARAM
#endif

// The pooling's gradient of the positions (sgg.h sgg_pool_dpos): one wave per
// ped r, the lanes over the 512 hidden units.  q(i, c) = g(i, c) sum_k W2[c, k]
// [hidden(i, j*, k) > 0] A[k, :] with j* = argmax[i, c] and g = dout where
// out > 0; dpos[r] = sum over the (i, c) of r's scene with j* = r, ascending,
// of q(i, c), minus sum_c q(r, c).
__global__ void __launch_bounds__(256) SGG_POOL_DPOS_KERNEL(const float* __restrict__ U, const float* __restrict__ pos,
                                                        const float* __restrict__ A, const float* __restrict__ W2,
                                                        const float* __restrict__ out,
                                                        const int32_t* __restrict__ am,
                                                        const float* __restrict__ dout,
                                                        const int32_t* __restrict__ scene_off, int S, int B, int bn,
                                                        float* __restrict__ dpos SGG_POOL_DROP_PARAM) {
#if SGG_POOL_DROP
  const PoolDropKey dk = pool_drop_key(drop);
#endif
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= B) return;
  // the scene of r: the last s with scene_off[s] <= r
  int lo = 0, hi = S - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (scene_off[mid] <= r) lo = mid; else hi = mid - 1;
  }
  const int i0 = scene_off[lo], i1 = scene_off[lo + 1];
  float a0[kHidden / 64], a1[kHidden / 64];
#pragma unroll
  for (int q = 0; q < kHidden / 64; ++q) {
    a0[q] = A[2 * (lane + 64 * q)];
    a1[q] = A[2 * (lane + 64 * q) + 1];
  }
  float sx = 0.f, sy = 0.f;   // identical in every lane
  // one (i, c) pair's q, times sign
  auto pair = [&](int i, int c, float sign) {
    const size_t o = (size_t)i * bn + c;
#if SGG_POOL_DROP
    const float g = out[o] > 0.f ? __fmul_rn(dout[o], dk.scale) : 0.f;
#else
    const float g = out[o] > 0.f ? dout[o] : 0.f;
#endif
    if (g == 0.f) return;
    const int j = am[o];
    const float dx = pos[2 * j] - pos[2 * i], dy = pos[2 * j + 1] - pos[2 * i + 1];
    float px = 0.f, py = 0.f;
#pragma unroll
    for (int q = 0; q < kHidden / 64; ++q) {
      const int k = lane + 64 * q;
      const float pre = fmaf(a1[q], dy, fmaf(a0[q], dx, U[(size_t)j * kHidden + k]));
#if SGG_POOL_DROP
      const float w = __fmul_rn(keep_if(W2[(size_t)c * kHidden + k], pre > 0.f),
                                pool_drop_factor(dk, SGG_POOL_DROP_SITE_HIDDEN, (uint32_t)i, (uint32_t)(j - i0), (uint32_t)k));
#else
      const float w = keep_if(W2[(size_t)c * kHidden + k], pre > 0.f);
#endif
      px = fmaf(w, a0[q], px);
      py = fmaf(w, a1[q], py);
    }
    sx = fmaf(sign * g, wave_sum(px), sx);
    sy = fmaf(sign * g, wave_sum(py), sy);
  };
  const int e0 = i0 * bn, e1 = i1 * bn;
  for (int base = e0; base < e1; base += 64) {
    const int e = base + lane;
    unsigned long long hits = __ballot(e < e1 && am[min(e, e1 - 1)] == r);
    while (hits) {
      const int b = __ffsll((long long)hits) - 1;
      hits &= hits - 1;
      const int eh = base + b;
      pair(eh / bn, eh % bn, 1.f);
    }
  }
  for (int c = 0; c < bn; ++c) pair(r, c, -1.f);
  if (lane == 0) {
    dpos[2 * r] = sx;
    dpos[2 * r + 1] = sy;
  }
}
