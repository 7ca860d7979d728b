// Adversarial loss of the training step (sgan/losses.py:5-21 bce_loss, as
// combined by gan_d_loss :36-49 / gan_g_loss :24-33 and weighted by the
// data-parallel shard fraction):
//   loss = w * ( mean_{i <  split} f(x_i, y_a) + mean_{i >= split} f(x_i, y_b) )
//   f(x, y) = max(x, 0) - x y + log(1 + exp(-|x|))
// The reference spends ~12 elementwise/reduction launches per bce_loss call
// plus their backward; here it is one launch forward and one backward.  The
// targets are device scalars so the step stays graph-capturable with fresh
// label-smoothing draws per replay.  nvalid (optional, device): only the
// first *nvalid scores of each half are real (a padded batch, PaddedScenes);
// the means run over those, the rest get a zero gradient.
#include "bce_body.h"
#include "sgg_common.h"

namespace sgg {

// d f / d x as torch's autograd forms it: clamp_min passes where x >= 0,
// abs' = sign(x) (0 at 0)
__device__ __forceinline__ float bce_grad(float x, float y) {
  const float e = expf(-fabsf(x));
  const float sg = x > 0.f ? 1.f : (x < 0.f ? -1.f : 0.f);
  return (x >= 0.f ? 1.f : 0.f) - y - sg * (e / (1.f + e));
}

// the value: bce_body.h's workgroup, the very code of the finish launch's BCE
// jobs (SggBceJob), hence the same bits
__global__ void __launch_bounds__(kBceThreads) bce_fwd_kernel(const SggBceJob d) {
  __shared__ float red[2][kBceThreads / 64];
  BceIn in;
  bce_load(d, in);
  const float addend = d.total ? *d.addend : 0.f;
  bce_value(d, in, addend, red);
}

__global__ void bce_bwd_kernel(const float* __restrict__ x, int n, int split, const float* __restrict__ ya,
                               const float* __restrict__ yb, float w, const float* __restrict__ gout,
                               float* __restrict__ dx, const int32_t* __restrict__ nvalid) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int nv = nvalid ? *nvalid : n;
  const bool first = i < split;
  const float cnt = first ? (float)min(split, nv) : (float)min(n - split, nv);
  dx[i] = bce_live(i, split, nv) ? (*gout * w / cnt) * bce_grad(x[i], first ? *ya : *yb) : 0.f;
}

}  // namespace sgg

using namespace sgg;

extern "C" int sgg_bce_fwd(const float* x, int n, int split, const float* ya, const float* yb, float w, float* loss,
                           const float* addend, float* total, const int32_t* nvalid, void* stream) {
  SGG_CHECK_ARG(loss && ya && yb && (n == 0 || x), "sgg_bce_fwd: null pointer");
  SGG_CHECK_ARG(!total || addend, "sgg_bce_fwd: total needs the addend");
  SGG_CHECK_ARG(n >= 0 && split >= 0 && split <= n, "sgg_bce_fwd: bad sizes n=%d split=%d", n, split);
  const SggBceJob d = {x, n, split, ya, yb, w, loss, addend, total, nvalid};
  hipLaunchKernelGGL(bce_fwd_kernel, dim3(1), dim3(kBceThreads), 0, (hipStream_t)stream, d);
  SGG_RETURN_LAUNCH("sgg_bce_fwd");
}

extern "C" int sgg_bce_bwd(const float* x, int n, int split, const float* ya, const float* yb, float w,
                           const float* gout, float* dx, const int32_t* nvalid, void* stream) {
  SGG_CHECK_ARG(ya && yb && gout && (n == 0 || (x && dx)), "sgg_bce_bwd: null pointer");
  SGG_CHECK_ARG(n >= 0 && split >= 0 && split <= n, "sgg_bce_bwd: bad sizes n=%d split=%d", n, split);
  if (n == 0) return 0;
  hipLaunchKernelGGL(bce_bwd_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, x, n, split, ya, yb,
                     w, gout, dx, nvalid);
  SGG_RETURN_LAUNCH("sgg_bce_bwd");
}
