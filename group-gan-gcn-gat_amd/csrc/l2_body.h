// The bodies of the two per-scene L2 glue kernels (glue.hip: sgg_l2_select,
// sgg_l2_loss_bwd_scenes), shared by their stand-alone kernels and by the glue
// workgroups of the four-wave LSTM forward launch (lstm_mw.hip,
// sgg_lstm_fwd_seg_glue).  The hosting kernel passes the virtual block index
// (the scene), its number of waves and the LDS it lends; every sum runs in an
// order that does not depend on the host's wave count, so both users produce
// the same bits.
#pragma once
#include "sgg_common.h"

namespace sgg {

// Both L2 kernels walk a scene's (step, ped) elements PED-FASTEST, so the gt
// and pred reads of a wave are contiguous runs (gt / pred are step-major:
// [T][B][2]); the scene's loss-mask block (ped-major, [B][ldm]) is first
// staged in LDS with coalesced reads and then read at (ped, step).
constexpr int kL2MaxElems = SGG_POOL_MAX_PEDS * 32;   // n * T staged per scene (larger: read in place)
constexpr int kL2MaxK = 256;                          // samples of sgg_l2_select (one LDS float each)

// the scene's mask block -> msk[i * T + t] (coalesced: t fastest)
__device__ __forceinline__ void stage_mask(float* msk, const float* __restrict__ mask, int ldm, int o, int n, int T,
                                           int t0, int nt) {
  for (int e = t0; e < n * T; e += nt) {
    const int i = e / T, t = e - i * T;
    msk[e] = mask[(size_t)(o + i) * ldm + t];
  }
}

// best-of-k of scene s by one workgroup of NW waves: wave w takes samples w,
// w + NW, ... (their loads together); lane = element, the sample's sum by a
// wave shuffle (over lanes and elements only: the same bits for every NW);
// argmin over the k samples (first minimum, as torch.argmin).  part: kL2MaxK
// floats, msk: kL2MaxElems floats of the workgroup's LDS; every thread of the
// workgroup calls it (two workgroup barriers).
template <int NW>
__device__ __forceinline__ void l2_select_body(const float* __restrict__ pred, const float* __restrict__ gt,
                                               const float* __restrict__ mask, int ldm,
                                               const int32_t* __restrict__ scene_off, int T, int B, int k,
                                               int64_t* __restrict__ best, int s, float* part, float* msk) {
  const int o = scene_off[s], n = scene_off[s + 1] - o;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float2* g2 = reinterpret_cast<const float2*>(gt);
  const float2* p2 = reinterpret_cast<const float2*>(pred);
  const int tot = n * T;
  const bool staged = tot <= kL2MaxElems;   // uniform
  if (staged) stage_mask(msk, mask, ldm, o, n, T, threadIdx.x, NW * 64);
  __syncthreads();
  constexpr int kRS = 4;
  for (int r0 = wave; r0 < k; r0 += NW * kRS) {
    float acc[kRS];
#pragma unroll
    for (int j = 0; j < kRS; ++j) acc[j] = 0.f;
    // four elements per lane in flight (a 20-ped scene's 240 in one round trip);
    // the sum runs over e = lane, lane + 64, ... in order, as with any unroll
    for (int e0 = lane; e0 < tot; e0 += 256) {
      float mk[4];
      float2 g[4], q[kRS][4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int e = min(e0 + 64 * u, tot - 1);
        const int t = e / n, i = e - t * n, p = o + i;
        mk[u] = staged ? msk[i * T + t] : mask[(size_t)p * ldm + t];
        g[u] = g2[(size_t)t * B + p];
#pragma unroll
        for (int j = 0; j < kRS; ++j) {
          const int r = min(r0 + NW * j, k - 1);
          q[j][u] = p2[((size_t)t * k + r) * B + p];
        }
      }
#pragma unroll
      for (int j = 0; j < kRS; ++j)
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (e0 + 64 * u < tot) {
            const float dx = g[u].x - q[j][u].x, dy = g[u].y - q[j][u].y;
            acc[j] = fmaf(mk[u], fmaf(dx, dx, dy * dy), acc[j]);
          }
    }
#pragma unroll
    for (int j = 0; j < kRS; ++j) {
      const float a = wave_sum(acc[j]);
      if (lane == 0 && r0 + NW * j < k) part[r0 + NW * j] = a;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int bi = 0;
    float bv = part[0];
    for (int r = 1; r < k; ++r)
      if (part[r] < bv) {
        bv = part[r];
        bi = r;
      }
    best[s] = bi;
  }
}

// one wave: the (masked squared error, mask) sums of scene [o, o + n); msk is
// the wave's own LDS staging buffer (kL2MaxElems)
__device__ __forceinline__ void l2_scene(const float* __restrict__ pred, int ldp, const float2* __restrict__ g2,
                                         const float* __restrict__ mask, int ldm, int o, int n, int T, int B,
                                         float* msk, int lane, float& acc_out, float& ms_out) {
  const int tot = n * T;
  const bool staged = tot <= kL2MaxElems;   // uniform
  if (staged) stage_mask(msk, mask, ldm, o, n, T, lane, 64);
  // lanes read entries other lanes wrote: a wavefront-scope release / acquire
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  float acc = 0.f, ms = 0.f;
  for (int e0 = lane; e0 < tot; e0 += 256) {
    float mk[4];
    float2 g[4], q[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int e = min(e0 + 64 * u, tot - 1);
      const int t = e / n, i = e - t * n, p = o + i;
      mk[u] = staged ? msk[i * T + t] : mask[(size_t)p * ldm + t];
      g[u] = g2[(size_t)t * B + p];
      q[u] = *reinterpret_cast<const float2*>(pred + (size_t)t * ldp + 2 * p);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (e0 + 64 * u < tot) {
        const float dx = g[u].x - q[u].x, dy = g[u].y - q[u].y;
        acc = fmaf(mk[u], fmaf(dx, dx, dy * dy), acc);
        ms += mk[u];
      }
  }
  acc_out = wave_sum(acc);
  ms_out = wave_sum(ms);
  // the staging buffer is rewritten by the wave's next scene: every lane's
  // reads of it are done (wave_sum consumed them) before the next stores
  __builtin_amdgcn_wave_barrier();
}

// sgg_l2_loss_bwd_scenes of scene s by ONE wave (lane = its lane; no
// workgroup barrier: a host with more waves lets the others return): the
// scene's mask sum as l2_terms_kernel forms it (same per-lane order, the same
// bits as the forward's msum), then the scene's rows of dpred with
// l2_loss_bwd_kernel's expression.  msk: kL2MaxElems floats of LDS.
__device__ __forceinline__ void l2_bwd_scene_body(const float* __restrict__ pred, int ldp,
                                                  const float* __restrict__ gt, const float* __restrict__ mask,
                                                  int ldm, const int32_t* __restrict__ scene_off, int T, int B,
                                                  float w, const float* __restrict__ gout,
                                                  float* __restrict__ dpred, int ldd, float* __restrict__ term, int s,
                                                  int lane, float* msk) {
  const int o = scene_off[s], n = scene_off[s + 1] - o;
  float acc, ms;
  l2_scene(pred, ldp, reinterpret_cast<const float2*>(gt), mask, ldm, o, n, T, B, msk, lane, acc, ms);
  if (term && lane == 0) term[s] = ms > 0.f ? (w * acc) / ms : 0.f;   // (l2_terms_kernel's value)
  const float g = *gout * w * -2.f;
  const float2* g2 = reinterpret_cast<const float2*>(gt);
  for (int e = lane; e < n * T; e += 64) {
    const int t = e / n, p = o + (e - t * n);
    const float m = mask[(size_t)p * ldm + t];
    const float2 gv = g2[(size_t)t * B + p];
    const float2 q = *reinterpret_cast<const float2*>(pred + (size_t)t * ldp + 2 * p);
    const float c = ms > 0.f ? g * m / ms : 0.f;
    *reinterpret_cast<float2*>(dpred + (size_t)t * ldd + 2 * p) = make_float2(c * (gv.x - q.x), c * (gv.y - q.y));
  }
}

}  // namespace sgg
