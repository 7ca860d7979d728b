// The row-local decoder step of the per-step pooling rollout
// (pool_every_timestep = 1, models.py:157-175), forward and backward, and the
// pooling's gradient of the positions.
//
// Between two poolings everything the reference's decoder does is row-local:
// decoder.mlp on [h | pool_h], the LSTM cell on the embedded displacement,
// hidden2pos, the new position, and the pooling net's first layer on the new
// h.  The pooling itself is an all-to-all seam over a scene's peds and stays
// its own launch (pool.hip / pool_wide.hip, unchanged); one launch here runs
// what lies between two seams.
//
// Workgroup = 4 waves = one tile of 16 peds.  Every product is the 16-row x
// 64-col wave tile of xw_body.h on v_mfma_f32_16x16x4_f32 (exact fp32), the
// waves taking the output columns 64 at a time; the tile's activations pass
// from one product to the next through two LDS buffers.  Sizes are runtime
// values: one forward and one backward kernel for every shape sgg_dec_step_ok
// takes.  Rows past B compute on a clamped (valid) row and store nothing.
#include "sgg_common.h"
#include "xw_body.h"
#include "pool_drop.h"

namespace sgg {

constexpr int kDsRows = 16;
constexpr int kDsMaxCols = 256;             // 4 H and mlp_dim at most
constexpr int kDsPitch = kDsMaxCols + 4;    // rows stay 16-byte aligned

// acc += X[16 rows, 0..K) Wop[0..K, col0 .. col0 + 64): xrow = this lane's row
// of X (global or LDS, 16-byte aligned when vec), W as sgg_xw takes it
template <bool TRANS_W>
__device__ __forceinline__ void ds_tile(const float* xrow, bool vec, int K, const float* W, int ldw, int N, int col0,
                                        floatx4 (&acc)[4]) {
  const int lane = threadIdx.x & 63;
  XwFrag<TRANS_W, false> f;
  f.xrow = xrow;
  f.mrow = nullptr;
  f.W = W;
  f.ws = nullptr;
  f.ldw = ldw;
  f.kp = 0;
  f.kend = K;
  f.kq = lane >> 4;
  f.vec = vec;
#pragma unroll
  for (int t = 0; t < 4; ++t) f.ncl[t] = min(col0 + 16 * t + (lane & 15), N - 1);
  xw_walk(f, 0, acc);
}

__device__ __forceinline__ void ds_zero(floatx4 (&acc)[4]) {
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = floatx4{0.f, 0.f, 0.f, 0.f};
}

__device__ __forceinline__ bool ds_al16(const void* p, int ld) {
  return ((reinterpret_cast<uintptr_t>(p) | (uintptr_t)ld * 4) & 15) == 0;
}

__device__ __forceinline__ float ds_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

__global__ void __launch_bounds__(256) dec_step_fwd_kernel(SggDecStep a) {
  __shared__ __attribute__((aligned(16))) float bufA[kDsRows * kDsPitch];
  __shared__ __attribute__((aligned(16))) float bufB[kDsRows * kDsPitch];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ar = lane & 15, kq = lane >> 4;
  const int B = a.B, H = a.H, bn = a.bn, D = a.mlp_dim;
  const int row0 = blockIdx.x * kDsRows;
  const int rl = min(row0 + ar, B - 1);   // the row this lane loads as the A operand
  floatx4 acc[4];

  if (a.mlp) {
    // z1 = relu([h_prev | pool_prev] W1m^T + b1m): the two input blocks in place
    const int ld1 = H + bn;
    for (int col0 = wave * 64; col0 < D; col0 += 256) {
      ds_zero(acc);
      ds_tile<true>(a.h_prev + (size_t)rl * H, ds_al16(a.h_prev, H), H, a.W1m, ld1, D, col0, acc);
      ds_tile<true>(a.pool_prev + (size_t)rl * bn, ds_al16(a.pool_prev, bn), bn, a.W1m + H, ld1, D, col0, acc);
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int n = col0 + 16 * t + ar;
        if (n >= D) continue;
        const float b = a.b1m[n];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int m = kq * 4 + r;
          const float v = fmaxf(acc[t][r] + b, 0.f);
          bufA[m * kDsPitch + n] = v;
          if (a.z1 && row0 + m < B) a.z1[(size_t)(row0 + m) * D + n] = v;
        }
      }
    }
    __syncthreads();
    // h_mix = relu(z1 W2m^T + b2m)
    for (int col0 = wave * 64; col0 < H; col0 += 256) {
      ds_zero(acc);
      ds_tile<true>(bufA + ar * kDsPitch, true, D, a.W2m, D, H, col0, acc);
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int n = col0 + 16 * t + ar;
        if (n >= H) continue;
        const float b = a.b2m[n];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int m = kq * 4 + r;
          const float v = fmaxf(acc[t][r] + b, 0.f);
          bufB[m * kDsPitch + n] = v;
          if (row0 + m < B) {
            if (a.h_mix) a.h_mix[(size_t)(row0 + m) * H + n] = v;
            if (!a.cell) a.h[(size_t)(row0 + m) * H + n] = v;
          }
        }
      }
    }
  } else {
    for (int e = threadIdx.x; e < kDsRows * H; e += 256) {
      const int m = e / H, u = e - m * H;
      const float v = a.h_prev[(size_t)min(row0 + m, B - 1) * H + u];
      bufB[m * kDsPitch + u] = v;
      if (a.h_mix && row0 + m < B) a.h_mix[(size_t)(row0 + m) * H + u] = v;   // (the W_hh gradient's operand)
    }
  }
  if (!a.cell) return;
  __syncthreads();

  // gates = A r_in + W_hh h_mix + bias (the input embedding folded into A)
  const int G4 = 4 * H;
  for (int col0 = wave * 64; col0 < G4; col0 += 256) {
    ds_zero(acc);
    ds_tile<true>(bufB + ar * kDsPitch, true, H, a.Whh, H, G4, col0, acc);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int n = col0 + 16 * t + ar;
      if (n >= G4) continue;
      const float b = a.bias[n], a0 = a.A[2 * n], a1 = a.A[2 * n + 1];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = kq * 4 + r;
        const float* rin = a.r_in + (size_t)min(row0 + m, B - 1) * 2;
        bufA[m * kDsPitch + n] = acc[t][r] + (b + fmaf(a1, rin[1], a0 * rin[0]));
      }
    }
  }
  __syncthreads();

  // the cell: c = f c_prev + i g, h = o tanh(c)  (gate order i, f, g, o)
  for (int e = threadIdx.x; e < kDsRows * H; e += 256) {
    const int m = e / H, u = e - m * H;
    const int row = min(row0 + m, B - 1);
    const float* g = bufA + m * kDsPitch;
    const float gi = ds_sigmoid(g[u]), gf = ds_sigmoid(g[H + u]), gg = tanhf(g[2 * H + u]), go = ds_sigmoid(g[3 * H + u]);
    const float cp = a.c_prev ? a.c_prev[(size_t)row * H + u] : 0.f;
    const float c = fmaf(gf, cp, gi * gg);
    const float h = go * tanhf(c);
    bufB[m * kDsPitch + u] = h;
    if (row0 + m < B) {
      a.h[(size_t)row * H + u] = h;
      a.c[(size_t)row * H + u] = c;
      if (a.act) {
        float* s = a.act + (size_t)row * G4;
        s[u] = gi;
        s[H + u] = gf;
        s[2 * H + u] = gg;
        s[3 * H + u] = go;
      }
    }
  }
  __syncthreads();

  // rel = Wp h + bp, pos = pos_prev + rel
  if (threadIdx.x < 2 * kDsRows) {
    const int m = threadIdx.x >> 1, k = threadIdx.x & 1;
    if (row0 + m < B) {
      float s = 0.f;
      for (int u = 0; u < H; ++u) s = fmaf(bufB[m * kDsPitch + u], a.Wp[k * H + u], s);
      s += a.bp[k];
      const size_t o = (size_t)(row0 + m) * 2 + k;
      a.rel[o] = s;
      a.pos[o] = a.pos_prev[o] + s;
    }
  }
  // U = h Wu^T + cu: the pooling net's first layer on h
  if (a.U) {
    for (int col0 = wave * 64; col0 < a.NU; col0 += 256) {
      ds_zero(acc);
      ds_tile<true>(bufB + ar * kDsPitch, true, H, a.Wu, a.ldwu, a.NU, col0, acc);
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int n = col0 + 16 * t + ar;
        if (n >= a.NU) continue;
        const float b = a.cu[n];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int m = row0 + kq * 4 + r;
          if (m < B) a.U[(size_t)m * a.NU + n] = acc[t][r] + b;
        }
      }
    }
  }
}

__global__ void __launch_bounds__(256) dec_step_bwd_kernel(SggDecStepBwd a) {
  __shared__ __attribute__((aligned(16))) float bufA[kDsRows * kDsPitch];
  __shared__ __attribute__((aligned(16))) float bufB[kDsRows * kDsPitch];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ar = lane & 15, kq = lane >> 4;
  const int B = a.B, H = a.H, bn = a.bn, D = a.mlp_dim;
  const int G4 = 4 * H;
  const int row0 = blockIdx.x * kDsRows;
  floatx4 acc[4];

  if (a.cell) {
    // drel_tot = drel + dpos; dh += Wp^T drel_tot; the cell backward -> dG
    for (int e = threadIdx.x; e < kDsRows * H; e += 256) {
      const int m = e / H, u = e - m * H;
      const int row = min(row0 + m, B - 1);
      const size_t o2 = (size_t)row * 2, oh = (size_t)row * H + u;
      const float dr0 = (a.drel ? a.drel[o2] : 0.f) + (a.dpos ? a.dpos[o2] : 0.f);
      const float dr1 = (a.drel ? a.drel[o2 + 1] : 0.f) + (a.dpos ? a.dpos[o2 + 1] : 0.f);
      const float dh = (a.dh ? a.dh[oh] : 0.f) + fmaf(a.Wp[H + u], dr1, a.Wp[u] * dr0);
      const float* s = a.act + (size_t)row * G4;
      const float gi = s[u], gf = s[H + u], gg = s[2 * H + u], go = s[3 * H + u];
      const float tc = tanhf(a.c[oh]);
      const float cp = a.c_prev ? a.c_prev[oh] : 0.f;
      const float dc = (a.dc ? a.dc[oh] : 0.f) + dh * go * (1.f - tc * tc);
      const float d[4] = {dc * gg * gi * (1.f - gi), dc * cp * gf * (1.f - gf), dc * gi * (1.f - gg * gg),
                          dh * tc * go * (1.f - go)};
#pragma unroll
      for (int q = 0; q < 4; ++q) bufA[m * kDsPitch + q * H + u] = d[q];
      if (row0 + m < B) {
#pragma unroll
        for (int q = 0; q < 4; ++q) a.dG[(size_t)row * G4 + q * H + u] = d[q];
        a.dc_prev[oh] = dc * gf;
        if (u < 2) {
          const float v = u ? dr1 : dr0;
          a.drel_tot[o2 + u] = v;
          if (a.dpos_prev) a.dpos_prev[o2 + u] = a.dpos ? a.dpos[o2 + u] : 0.f;
        }
      }
    }
    __syncthreads();
    // dr_in = dG A
    if (threadIdx.x < 2 * kDsRows) {
      const int m = threadIdx.x >> 1, k = threadIdx.x & 1;
      if (row0 + m < B) {
        float s = 0.f;
        for (int n = 0; n < G4; ++n) s = fmaf(bufA[m * kDsPitch + n], a.A[2 * n + k], s);
        a.dr_in[(size_t)(row0 + m) * 2 + k] = s;
      }
    }
    // dh_mix = dG W_hh
    for (int col0 = wave * 64; col0 < H; col0 += 256) {
      ds_zero(acc);
      ds_tile<false>(bufA + ar * kDsPitch, true, G4, a.Whh, H, H, col0, acc);
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int n = col0 + 16 * t + ar;
        if (n >= H) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int m = kq * 4 + r;
          const int row = min(row0 + m, B - 1);
          float v = acc[t][r];
          if (a.mlp) {
            v = keep_if(v, a.h_mix[(size_t)row * H + n] > 0.f);
            bufB[m * kDsPitch + n] = v;
            if (row0 + m < B) a.dz2[(size_t)row * H + n] = v;
          } else if (row0 + m < B) {
            a.dh_prev[(size_t)row * H + n] = v;
          }
        }
      }
    }
  } else {
    // the tail form: dh is the gradient of h_mix
    for (int e = threadIdx.x; e < kDsRows * H; e += 256) {
      const int m = e / H, u = e - m * H;
      const int row = min(row0 + m, B - 1);
      const size_t oh = (size_t)row * H + u;
      const float v = keep_if(a.dh[oh], a.h_mix[oh] > 0.f);
      bufB[m * kDsPitch + u] = v;
      if (row0 + m < B) a.dz2[oh] = v;
    }
  }
  if (!a.mlp) return;
  __syncthreads();

  // dz1 = (dz2 W2m) where z1 > 0
  for (int col0 = wave * 64; col0 < D; col0 += 256) {
    ds_zero(acc);
    ds_tile<false>(bufB + ar * kDsPitch, true, H, a.W2m, D, D, col0, acc);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int n = col0 + 16 * t + ar;
      if (n >= D) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = kq * 4 + r;
        const int row = min(row0 + m, B - 1);
        const float v = keep_if(acc[t][r], a.z1[(size_t)row * D + n] > 0.f);
        bufA[m * kDsPitch + n] = v;
        if (row0 + m < B) a.dz1[(size_t)row * D + n] = v;
      }
    }
  }
  __syncthreads();
  // [dh_prev | dpool_prev] = dz1 W1m
  const int ld1 = H + bn;
  for (int col0 = wave * 64; col0 < ld1; col0 += 256) {
    ds_zero(acc);
    ds_tile<false>(bufA + ar * kDsPitch, true, D, a.W1m, ld1, ld1, col0, acc);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int n = col0 + 16 * t + ar;
      if (n >= ld1) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = row0 + kq * 4 + r;
        if (m >= B) continue;
        if (n < H)
          a.dh_prev[(size_t)m * H + n] = acc[t][r];
        else
          a.dpool_prev[(size_t)m * bn + (n - H)] = acc[t][r];
      }
    }
  }
}

// pool_dpos_kernel and its dropout form pool_dpos_drop_kernel: one text (pool_dpos_kernel.h) compiled twice
#define SGG_POOL_DROP 0
#include "pool_dpos_kernel.h"
#undef SGG_POOL_DROP
#define SGG_POOL_DROP 1
#include "pool_dpos_kernel.h"
#undef SGG_POOL_DROP

static bool ds_cell_ok(int H, int NU) { return H >= 16 && H <= 64 && H % 16 == 0 && (NU == 0 || NU == kHidden); }
static bool ds_mlp_ok(int H, int bn, int D) { return bn >= 1 && H + bn <= kDsMaxCols && D >= 1 && D <= kDsMaxCols; }

}  // namespace sgg

extern "C" {

int sgg_dec_step_ok(int H, int bn, int mlp_dim, int NU) {
  if (!sgg::ds_cell_ok(H, NU)) return 0;
  return sgg::ds_mlp_ok(H, bn, mlp_dim) ? 3 : 1;
}

long long sgg_dec_step_saved_floats(int B, int H, int mlp_dim) {
  if (B < 0 || H < 0 || mlp_dim < 0) return 0;
  const long long n = (long long)B * (5LL * H + mlp_dim);
  return (n + 3) / 4 * 4;
}

int sgg_dec_step_fwd(const SggDecStep* a, void* stream) {
  SGG_CHECK_ARG(a != nullptr, "sgg_dec_step_fwd: NULL arguments");
  SGG_CHECK_ARG(a->B >= 0, "sgg_dec_step_fwd: B = %d", a->B);
  SGG_CHECK_ARG(sgg::ds_cell_ok(a->H, a->U ? a->NU : 0), "sgg_dec_step_fwd: H = %d, NU = %d not built", a->H, a->NU);
  SGG_CHECK_ARG(a->cell || a->mlp, "sgg_dec_step_fwd: neither the cell nor the mlp part is on");
  SGG_CHECK_ARG(!a->mlp || sgg::ds_mlp_ok(a->H, a->bn, a->mlp_dim), "sgg_dec_step_fwd: mlp bn = %d, mlp_dim = %d out of bounds",
                a->bn, a->mlp_dim);
  SGG_CHECK_ARG(a->h_prev && a->h, "sgg_dec_step_fwd: h_prev / h is NULL");
  SGG_CHECK_ARG(!a->mlp || (a->pool_prev && a->W1m && a->b1m && a->W2m && a->b2m), "sgg_dec_step_fwd: mlp operand is NULL");
  SGG_CHECK_ARG(!a->cell || (a->r_in && a->pos_prev && a->A && a->Whh && a->bias && a->Wp && a->bp && a->c && a->rel &&
                             a->pos),
                "sgg_dec_step_fwd: cell operand is NULL");
  SGG_CHECK_ARG(!a->U || (a->cell && a->Wu && a->cu && a->ldwu >= a->H), "sgg_dec_step_fwd: U needs the cell, Wu, cu, ldwu >= H");
  if (a->B == 0) return 0;
  hipLaunchKernelGGL(sgg::dec_step_fwd_kernel, dim3((a->B + 15) / 16), dim3(256), 0, (hipStream_t)stream, *a);
  SGG_RETURN_LAUNCH("sgg_dec_step_fwd");
}

int sgg_dec_step_bwd(const SggDecStepBwd* a, void* stream) {
  SGG_CHECK_ARG(a != nullptr, "sgg_dec_step_bwd: NULL arguments");
  SGG_CHECK_ARG(a->B >= 0, "sgg_dec_step_bwd: B = %d", a->B);
  SGG_CHECK_ARG(sgg::ds_cell_ok(a->H, 0), "sgg_dec_step_bwd: H = %d not built", a->H);
  SGG_CHECK_ARG(a->cell || a->mlp, "sgg_dec_step_bwd: neither the cell nor the mlp part is on");
  SGG_CHECK_ARG(!a->mlp || sgg::ds_mlp_ok(a->H, a->bn, a->mlp_dim), "sgg_dec_step_bwd: mlp bn = %d, mlp_dim = %d out of bounds",
                a->bn, a->mlp_dim);
  SGG_CHECK_ARG(!a->cell || (a->act && a->c && a->A && a->Whh && a->Wp && a->dG && a->dc_prev && a->dr_in && a->drel_tot),
                "sgg_dec_step_bwd: cell operand is NULL");
  SGG_CHECK_ARG(a->cell || a->dh, "sgg_dec_step_bwd: the tail form needs dh");
  SGG_CHECK_ARG(!a->mlp || (a->h_mix && a->z1 && a->W1m && a->W2m && a->dz2 && a->dz1 && a->dh_prev && a->dpool_prev),
                "sgg_dec_step_bwd: mlp operand is NULL");
  SGG_CHECK_ARG(a->mlp || a->dh_prev, "sgg_dec_step_bwd: dh_prev is NULL");
  if (a->B == 0) return 0;
  hipLaunchKernelGGL(sgg::dec_step_bwd_kernel, dim3((a->B + 15) / 16), dim3(256), 0, (hipStream_t)stream, *a);
  SGG_RETURN_LAUNCH("sgg_dec_step_bwd");
}

int sgg_pool_dpos(const float* U, const float* pos, const float* A, const float* W2, const float* out,
                  const int32_t* argmax, const float* dout, const int32_t* scene_off, int S, int B, int bn,
                  float* dpos, void* stream) {
  SGG_CHECK_ARG(U && pos && A && W2 && out && argmax && dout && scene_off && dpos, "sgg_pool_dpos: NULL operand");
  SGG_CHECK_ARG(S >= 1 && B >= 0 && bn >= 1, "sgg_pool_dpos: S = %d, B = %d, bn = %d", S, B, bn);
  if (B == 0) return 0;
  hipLaunchKernelGGL(sgg::pool_dpos_kernel, dim3((B + 3) / 4), dim3(256), 0, (hipStream_t)stream, U, pos, A, W2, out,
                     argmax, dout, scene_off, S, B, bn, dpos);
  SGG_RETURN_LAUNCH("sgg_pool_dpos");
}

int sgg_pool_dpos_drop(const float* U, const float* pos, const float* A, const float* W2, const float* out,
                       const int32_t* argmax, const float* dout, const int32_t* scene_off, int S, int B, int bn,
                       float* dpos, float p, unsigned long long seed, unsigned offset,
                       const unsigned long long* rng_dev, void* stream) {
  SGG_CHECK_ARG(U && pos && A && W2 && out && argmax && dout && scene_off && dpos, "sgg_pool_dpos_drop: NULL operand");
  SGG_CHECK_ARG(S >= 1 && B >= 0 && bn >= 1 && bn <= SGG_POOL_BN_MAX, "sgg_pool_dpos_drop: S = %d, B = %d, bn = %d (1 .. %d)",
                S, B, bn, SGG_POOL_BN_MAX);
  sgg::DropArgs d;
  if (!sgg::pool_drop_args("sgg_pool_dpos_drop", p, seed, offset, rng_dev, &d)) return SGG_E_ARG;
  if (B == 0) return 0;
  hipLaunchKernelGGL(sgg::pool_dpos_drop_kernel, dim3((B + 3) / 4), dim3(256), 0, (hipStream_t)stream, U, pos, A, W2,
                     out, argmax, dout, scene_off, S, B, bn, dpos, d);
  SGG_RETURN_LAUNCH("sgg_pool_dpos_drop");
}

}  // extern "C"
