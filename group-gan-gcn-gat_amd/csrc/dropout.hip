// Feature dropout (F.dropout on a node-feature matrix: GAT.forward,
// reference sgan/models.py:233, 235; the batched GAT's between-layer dropout,
// sgan/GAT.py:87 text): y = keep ? x * scale : 0 with the stateless mask of
// dropout_common.h (head 0, column = feature column), so the backward is the
// same call on dy.
#include "sgg_common.h"
#include "dropout_common.h"

namespace sgg {

constexpr int kDropThreads = 256;

// One work item = 4 rows x 4 columns: the four rows of a Philox call (rows
// 4 rq .. 4 rq + 3 share the counter) at four adjacent columns, so a call's
// words are all used and a row's four values move as one 16-byte access when
// VEC (both strides multiples of 4, both bases 16-byte aligned); the last
// column group of a row, and every group otherwise, moves by elements.  Each
// element is read and written by one thread: y may be x.
template <bool VEC>
__global__ void __launch_bounds__(kDropThreads) dropout_kernel(const float* x, int ldx, int rows, int cols,
                                                               const DropArgs drop, float* y, int ldy) {
  const DropKey dk = drop_key(drop, 0);
  const int rqs = (rows + 3) >> 2, cqs = (cols + 3) >> 2;
  const long long items = (long long)rqs * cqs;
  for (long long it = (long long)blockIdx.x * kDropThreads + threadIdx.x; it < items;
       it += (long long)gridDim.x * kDropThreads) {
    const int rq = (int)(it / cqs), c0 = 4 * (int)(it - (long long)rq * cqs);
    float m[4][4];   // [row of the quad][column]: scale or 0
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const Philox4 w = drop_words(dk, (uint32_t)rq, (uint32_t)(c0 + c));
#pragma unroll
      for (int r = 0; r < 4; ++r) m[r][c] = w.w[r] >= dk.thr ? dk.scale : 0.f;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 4 * rq + r;
      if (row >= rows) break;
      const float* xr = x + (size_t)row * ldx + c0;
      float* yr = y + (size_t)row * ldy + c0;
      if (VEC && c0 + 4 <= cols) {
        const float4 v = *reinterpret_cast<const float4*>(xr);
        // (a dropped value is exactly 0, whatever x holds)
        const float* mr = m[r];
        *reinterpret_cast<float4*>(yr) = float4{mr[0] != 0.f ? v.x * mr[0] : 0.f, mr[1] != 0.f ? v.y * mr[1] : 0.f,
                                                mr[2] != 0.f ? v.z * mr[2] : 0.f, mr[3] != 0.f ? v.w * mr[3] : 0.f};
      } else {
#pragma unroll
        for (int c = 0; c < 4; ++c)
          if (c0 + c < cols) yr[c] = m[r][c] != 0.f ? xr[c] * m[r][c] : 0.f;
      }
    }
  }
}

}  // namespace sgg

using namespace sgg;

extern "C" int sgg_dropout(const float* x, int ldx, int rows, int cols, float p, unsigned long long seed,
                           unsigned offset, unsigned site, const unsigned long long* rng_dev, float* y, int ldy,
                           void* stream) {
  SGG_CHECK_ARG(x && y, "sgg_dropout: null pointer");
  SGG_CHECK_ARG(rows >= 0 && cols >= 0 && ldx >= cols && ldy >= cols, "sgg_dropout: bad sizes");
  SGG_CHECK_ARG(p >= 0.f && p < 1.f, "sgg_dropout: dropout p=%g outside [0, 1)", (double)p);
  SGG_CHECK_ARG(site < (1u << 24), "sgg_dropout: dropout site %u is not below 2^24", site);
  SGG_CHECK_ARG(((uintptr_t)rng_dev & 7) == 0, "sgg_dropout: rng_dev must be 8-byte aligned");
  if (rows == 0 || cols == 0) return 0;
  const DropArgs d{seed, rng_dev, offset, site, 0u, drop_threshold(p), drop_scale(p)};
  const long long items = (long long)((rows + 3) >> 2) * ((cols + 3) >> 2);
  const long long blocks = (items + kDropThreads - 1) / kDropThreads;
  const int grid = blocks < 4096 ? (int)blocks : 4096;
  const bool vec = ldx % 4 == 0 && ldy % 4 == 0 && ((uintptr_t)x & 15) == 0 && ((uintptr_t)y & 15) == 0;
  auto k = vec ? dropout_kernel<true> : dropout_kernel<false>;
  hipLaunchKernelGGL(k, dim3(grid), dim3(kDropThreads), 0, (hipStream_t)stream, x, ldx, rows, cols, d, y, ldy);
  SGG_RETURN_LAUNCH("sgg_dropout");
}
