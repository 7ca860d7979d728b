// Social pooling with batch norm in train(): mlp_pre_pool = Linear, BatchNorm1d, ReLU, Linear,
// BatchNorm1d, ReLU over the n x n pair rows of ONE scene (row i n + j = [E(p_j - p_i); h_j]),
// both BatchNorms on the scene's own biased statistics.  fp32 throughout, every bn in
// 1 .. SGG_POOL_BN_MAX, scenes of 2 .. SGG_POOL_NORM_MAX_PEDS peds.
// Nothing in LDS or registers grows with the scene: a workgroup walks a scene's pairs in tiles of 16.
//
// Forward (sgg_pool_norm_fwd), three launches on the one stream:
//   pool_norm_stats1_kernel  first-layer statistics in closed form from U, A and the positions
//                            (no pass over pairs), BatchNorm 1 folded into Un = g (U - mu) + beta,
//                            An = g A per scene
//   pool_norm_fwd_kernel<0>  y2 per pair tile, per column (count, mean, M2) merged tile by tile
//   pool_norm_fwd_kernel<1>  y2 again, g2 (y2 - mu2) + beta2, ReLU, max over j (smallest j on ties)
// Backward (sgg_pool_norm_bwd), two launches:
//   pool_norm_bwd_kernel     the dense pass over all pairs: dy2 tile, dA1 = dy2 W2, dW2 += a1^T dy2,
//                            the row / column sums R_j, C_i and G = sum dz1 (x) (p_j - p_i)
//   pool_norm_finish_kernel  BatchNorm 1's backward in closed form on R, C, G: dU, dpos, dA, dgamma1,
//                            dbeta1
// A workgroup owns whole scenes, every sum has one owner thread and a fixed order: no atomics of any
// kind, two runs are bitwise equal.  The pair tiles run on the vector ALU (16 pairs x 64 columns per
// step, W2 staged through LDS).
#include "sgg_common.h"
#include "pool_common.h"
#include <math.h>

namespace sgg {

constexpr int kNH = kHidden;       // hidden units = threads of a workgroup
constexpr int kNTP = 16;           // pairs of a tile
constexpr int kNCT = 64;           // columns of a tile
constexpr int kNKT = 64;           // hidden units of a staged W2 tile
constexpr int kNWS = kNCT + 1;     // its LDS row stride
constexpr int kNMaxN = SGG_POOL_NORM_MAX_PEDS;
constexpr int kNFinRows = SGG_POOL_NORM_FIN_ROWS;      // rows of the finish kernel's slab [dA | dgamma1 | dbeta1]
constexpr int kNFinCols = 4 * kNH;

// ---- first-layer statistics -----------------------------------------------------
// y1[i, j, k] = a_j - q_i with a_j = U[j, k] + p_j . A_k, q_i = p_i . A_k, so over the n x n grid
// mean = mean_j U[j, k] and var = var_j(a) + var_i(q) (biased), both centred sums over n peds.
__global__ void __launch_bounds__(512) pool_norm_stats1_kernel(
    const float* __restrict__ U, const float* __restrict__ pos, const float* __restrict__ A,
    const float* __restrict__ gamma1, const float* __restrict__ beta1, const int32_t* __restrict__ scene_off, int S,
    float eps, float* __restrict__ Un, float* __restrict__ An, float* __restrict__ mu1, float* __restrict__ var1) {
  const int k = threadIdx.x;
  const float ax = A[2 * k], ay = A[2 * k + 1];
  const float gam = gamma1[k], bet = beta1[k];
  for (int s = blockIdx.x; s < S; s += gridDim.x) {
    const int o = scene_off[s], n = scene_off[s + 1] - o;
    if (n < 1) continue;
    // (sums over a scene's peds: double accumulators, O(n) work per hidden unit)
    double su = 0.0, sq = 0.0;
    for (int j = 0; j < n; ++j) {
      su += (double)U[(size_t)(o + j) * kNH + k];
      sq += (double)fmaf(ay, pos[2 * (o + j) + 1], ax * pos[2 * (o + j)]);
    }
    const double inv = 1.0 / (double)n;
    const float mu = (float)(su * inv), mq = (float)(sq * inv);
    double va = 0.0, vq = 0.0;
    for (int j = 0; j < n; ++j) {
      const float q = fmaf(ay, pos[2 * (o + j) + 1], ax * pos[2 * (o + j)]);
      const float da = (U[(size_t)(o + j) * kNH + k] - mu) + (q - mq), dq = q - mq;
      va += (double)da * (double)da;
      vq += (double)dq * (double)dq;
    }
    const float var = (float)((va + vq) * inv);
    const float g = gam / sqrtf(var + eps);
    for (int j = 0; j < n; ++j) Un[(size_t)(o + j) * kNH + k] = fmaf(g, U[(size_t)(o + j) * kNH + k] - mu, bet);
    An[(size_t)s * 2 * kNH + 2 * k] = g * ax;
    An[(size_t)s * 2 * kNH + 2 * k + 1] = g * ay;
    mu1[(size_t)s * kNH + k] = mu;
    var1[(size_t)s * kNH + k] = var;
  }
}

// ---- the pair tile (shared by the forward passes and the dense backward) ---------------
// a1 of pairs [p0, p0 + 16) of a scene (pair p = i n + j), hidden unit k = thread: into a1s[e][k]
// and the caller's registers; pairs >= M are 0.
__device__ __forceinline__ void norm_a1_tile(const float* __restrict__ Un, const float* __restrict__ pos, int o,
                                             int n, int M, int p0, float ax, float ay, float* a1s,
                                             float (&a1)[kNTP]) {
  const int k = threadIdx.x;
#pragma unroll
  for (int e = 0; e < kNTP; ++e) {
    const int p = p0 + e;
    float v = 0.f;
    if (p < M) {
      const int i = p / n, j = p - i * n;
      // (the positions: one address for the whole workgroup, read through the scalar cache)
      const float rx = pos[2 * (o + j)] - pos[2 * (o + i)], ry = pos[2 * (o + j) + 1] - pos[2 * (o + i) + 1];
      v = fmaxf(fmaf(ay, ry, fmaf(ax, rx, Un[(size_t)(o + j) * kNH + k])), 0.f);
    }
    a1[e] = v;
    a1s[e * kNH + k] = v;
  }
}

// y2 of the tile's pairs 2 pg, 2 pg + 1 (pg = thread / 64) in column cb + (thread % 64), bias
// included: hidden units ascending in one FMA chain.  Opens with a barrier (a1s written, the
// previous tile's LDS readers done); every thread must call it.
__device__ __forceinline__ void norm_y2_tile(const float* __restrict__ W2, const float* __restrict__ b2, int bn,
                                             int cb, const float* a1s, float* w2s, float& y0, float& y1) {
  const int t = threadIdx.x;
  const int c = t & 63, pg = t >> 6;
  const int cc = t >> 3, k8 = (t & 7) * 8;
  float acc0 = 0.f, acc1 = 0.f;
  for (int k0 = 0; k0 < kNH; k0 += kNKT) {
    float4 w0 = make_float4(0.f, 0.f, 0.f, 0.f), w1 = w0;
    if (cb + cc < bn) {
      const float4* src = reinterpret_cast<const float4*>(W2 + (size_t)(cb + cc) * kNH + k0 + k8);
      w0 = src[0];
      w1 = src[1];
    }
    __syncthreads();
    float* d = w2s + k8 * kNWS + cc;
    d[0] = w0.x; d[kNWS] = w0.y; d[2 * kNWS] = w0.z; d[3 * kNWS] = w0.w;
    d[4 * kNWS] = w1.x; d[5 * kNWS] = w1.y; d[6 * kNWS] = w1.z; d[7 * kNWS] = w1.w;
    __syncthreads();
    const float* r0 = a1s + (2 * pg) * kNH + k0;
    const float* r1 = r0 + kNH;
#pragma unroll 8
    for (int kk = 0; kk < kNKT; ++kk) {
      const float w = w2s[kk * kNWS + c];
      acc0 = fmaf(r0[kk], w, acc0);
      acc1 = fmaf(r1[kk], w, acc1);
    }
  }
  const float b = cb + c < bn ? b2[cb + c] : 0.f;
  y0 = acc0 + b;
  y1 = acc1 + b;
}

// ---- forward passes ---------------------------------------------------------------
// workgroup (x, y): scenes x, x + gridDim.x, .. against columns [64 y, 64 y + 64).
// APPLY = false: mu2 / var2 of the scene's columns -- per tile the 16 values' mean and centred M2,
// merged into the running (count, mean, M2) (Chan), tiles ascending.
// APPLY = true: out / argmax.  The affine map comes before the max (gamma2 may be negative).
template <bool APPLY>
__global__ void __launch_bounds__(512) pool_norm_fwd_kernel(
    const float* __restrict__ Un, const float* __restrict__ pos, const float* __restrict__ An,
    const float* __restrict__ W2, const float* __restrict__ b2, const float* __restrict__ gamma2,
    const float* __restrict__ beta2, const int32_t* __restrict__ scene_off, int S, int bn, float eps,
    float* __restrict__ mu2, float* __restrict__ var2, float* __restrict__ out, int32_t* __restrict__ argmax) {
  __shared__ float a1s[kNTP * kNH];
  __shared__ float w2s[kNKT * kNWS];
  __shared__ float y2s[kNTP * kNCT];
  const int t = threadIdx.x, c = t & 63, pg = t >> 6;
  const int cb = (int)blockIdx.y * kNCT;
  const bool owner = t < kNCT && cb + c < bn;
  for (int s = blockIdx.x; s < S; s += gridDim.x) {
    const int o = scene_off[s], n = scene_off[s + 1] - o;
    if (n < 1 || n > kNMaxN) continue;
    const int M = n * n;
    const float ax = An[(size_t)s * 2 * kNH + 2 * t], ay = An[(size_t)s * 2 * kNH + 2 * t + 1];
    float cnt = 0.f, mean = 0.f, m2 = 0.f;          // statistics
    float g2 = 0.f, mu = 0.f, be = 0.f, best = -1.f;  // apply
    int bj = 0, cur = 0;
    if (APPLY && owner) {
      mu = mu2[(size_t)s * bn + cb + c];
      g2 = gamma2[cb + c] / sqrtf(var2[(size_t)s * bn + cb + c] + eps);
      be = beta2[cb + c];
    }
    for (int p0 = 0; p0 < M; p0 += kNTP) {
      float a1[kNTP], y0, y1;
      norm_a1_tile(Un, pos, o, n, M, p0, ax, ay, a1s, a1);
      norm_y2_tile(W2, b2, bn, cb, a1s, w2s, y0, y1);
      y2s[(2 * pg) * kNCT + c] = y0;
      y2s[(2 * pg + 1) * kNCT + c] = y1;
      __syncthreads();
      if (owner) {
        const int np = min(kNTP, M - p0);
        if (!APPLY) {
          float sm = 0.f;
          for (int e = 0; e < np; ++e) sm += y2s[e * kNCT + c];
          const float tm = sm / (float)np;
          float tq = 0.f;
          for (int e = 0; e < np; ++e) {
            const float d = y2s[e * kNCT + c] - tm;
            tq = fmaf(d, d, tq);
          }
          const float tot = cnt + (float)np, d = tm - mean;
          mean = fmaf(d, (float)np / tot, mean);
          m2 += tq + d * d * (cnt * (float)np / tot);
          cnt = tot;
        } else {
          for (int e = 0; e < np; ++e) {
            const int p = p0 + e, i = p / n, j = p - i * n;
            if (i != cur) {
              out[(size_t)(o + cur) * bn + cb + c] = best;
              argmax[(size_t)(o + cur) * bn + cb + c] = o + bj;
              best = -1.f;
              cur = i;
            }
            const float v = fmaxf(fmaf(g2, y2s[e * kNCT + c] - mu, be), 0.f);
            if (v > best) { best = v; bj = j; }
          }
        }
      }
    }
    if (owner) {
      if (!APPLY) {
        mu2[(size_t)s * bn + cb + c] = mean;
        var2[(size_t)s * bn + cb + c] = m2 / (float)M;
      } else {
        out[(size_t)(o + cur) * bn + cb + c] = best;
        argmax[(size_t)(o + cur) * bn + cb + c] = o + bj;
      }
    }
  }
}

// ---- running statistics ---------------------------------------------------------------
// r <- (1 - m) r + m stat_s, scene after scene as the module does; the variance unbiased
// (n^2 / (n^2 - 1)).  Thread = column.
__global__ void __launch_bounds__(256) pool_norm_running_kernel(
    const float* __restrict__ mean, const float* __restrict__ var, const int32_t* __restrict__ scene_off, int S, int C,
    float m, float* __restrict__ rmean, float* __restrict__ rvar) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  float rm = rmean[c], rv = rvar[c];
  for (int s = 0; s < S; ++s) {
    const int n = scene_off[s + 1] - scene_off[s];
    if (n < 2) continue;
    const float Mf = (float)n * (float)n;
    rm = fmaf(m, mean[(size_t)s * C + c], (1.f - m) * rm);
    rv = fmaf(m, var[(size_t)s * C + c] * (Mf / (Mf - 1.f)), (1.f - m) * rv);
  }
  rmean[c] = rm;
  rvar[c] = rv;
}

// ---- dense backward ---------------------------------------------------------------------
// Workgroup r owns slab row r = [dW2 (bn x 512) | dgamma2 | dbeta2] and the scenes r, r + rows, ..
// Per scene: the head (dbeta2 = sum dz, dgamma2 = sum dz yhat2 with yhat2 = (out - beta2) / gamma2 at
// the argmax row, dz = dout where out > 0), then every pair tile against every column tile:
//   dy2 = g2 (dz - dbeta2 / M - yhat2 dgamma2 / M)      (dz at the argmax pair only)
//   dA1[e][k] += sum_c dy2[e][c] W2[c][k]                (thread k, columns ascending)
//   slab[r][c][k] += sum_e dy2[e][c] a1[e][k]            (the owner thread's own read-modify-write)
// and after the last column tile dz1 = dA1 where a1 > 0 goes into R[j][k] (own read-modify-write),
// C[i][k] (a register until i changes; pairs are i-major) and G[k].
template <bool WGRAD>
__global__ void __launch_bounds__(512) pool_norm_bwd_kernel(
    const float* __restrict__ Un, const float* __restrict__ pos, const float* __restrict__ An,
    const float* __restrict__ W2, const float* __restrict__ b2, const float* __restrict__ gamma2,
    const float* __restrict__ beta2, const float* __restrict__ mu2, const float* __restrict__ var2,
    const float* __restrict__ out, const int32_t* __restrict__ argmax, const float* __restrict__ dout,
    const int32_t* __restrict__ scene_off, int S, int bn, float eps, float* slab, double* R, float* __restrict__ C,
    double* __restrict__ G) {
  __shared__ float a1s[kNTP * kNH];
  __shared__ float w2s[kNKT * kNWS];
  __shared__ float y2s[kNTP * kNCT];
  __shared__ float hg[SGG_POOL_BN_MAX], hb[SGG_POOL_BN_MAX];
  const int t = threadIdx.x, c = t & 63, pg = t >> 6;
  const size_t cols = (size_t)bn * kNH + 2 * bn;
  float* row = slab + (size_t)blockIdx.x * cols;
  if (WGRAD)
    for (size_t q = t; q < cols; q += 512) row[q] = 0.f;
  for (int s = blockIdx.x; s < S; s += gridDim.x) {
    const int o = scene_off[s], n = scene_off[s + 1] - o;
    if (n < 1 || n > kNMaxN) continue;
    const int M = n * n;
    const float invM = 1.f / (float)M;
    __syncthreads();   // the previous scene's readers of hg / hb done
    for (int cg = t; cg < bn; cg += 512) {
      const float gam = gamma2[cg], bet = beta2[cg];
      const float ig = gam != 0.f ? 1.f / gam : 0.f;
      float db = 0.f, dg = 0.f;
      for (int i = 0; i < n; ++i) {
        const float ov = out[(size_t)(o + i) * bn + cg];
        const float dz = ov > 0.f ? dout[(size_t)(o + i) * bn + cg] : 0.f;
        db += dz;
        dg = fmaf(dz, (ov - bet) * ig, dg);
      }
      hg[cg] = dg;
      hb[cg] = db;
      if (WGRAD) {
        row[(size_t)bn * kNH + cg] += dg;
        row[(size_t)bn * kNH + bn + cg] += db;
      }
    }
    for (int j = 0; j < n; ++j) R[(size_t)(o + j) * kNH + t] = 0.0;
    __syncthreads();
    const float ax = An[(size_t)s * 2 * kNH + 2 * t], ay = An[(size_t)s * 2 * kNH + 2 * t + 1];
    double gx = 0.0, gy = 0.0;   // (n^2 terms each: double accumulators)
    float cacc = 0.f;
    int cur = 0;
    for (int p0 = 0; p0 < M; p0 += kNTP) {
      float a1[kNTP], dA1[kNTP];
      norm_a1_tile(Un, pos, o, n, M, p0, ax, ay, a1s, a1);
#pragma unroll
      for (int e = 0; e < kNTP; ++e) dA1[e] = 0.f;
      for (int cb = 0; cb < bn; cb += kNCT) {
        float y[2];
        norm_y2_tile(W2, b2, bn, cb, a1s, w2s, y[0], y[1]);
        const int cg = cb + c;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int e = 2 * pg + h, p = p0 + e;
          float dy = 0.f;
          if (p < M && cg < bn) {
            const int i = p / n, j = p - i * n;
            const float rs = 1.f / sqrtf(var2[(size_t)s * bn + cg] + eps);
            const float yh = (y[h] - mu2[(size_t)s * bn + cg]) * rs;
            const size_t oi = (size_t)(o + i) * bn + cg;
            const float dz = (argmax[oi] == o + j && out[oi] > 0.f) ? dout[oi] : 0.f;
            dy = gamma2[cg] * rs * (dz - hb[cg] * invM - yh * hg[cg] * invM);
          }
          y2s[e * kNCT + c] = dy;
        }
        __syncthreads();
        const int nc = min(kNCT, bn - cb);
        for (int q = 0; q < nc; ++q) {
          const float w = W2[(size_t)(cb + q) * kNH + t];
          float acc = 0.f;
#pragma unroll
          for (int e = 0; e < kNTP; ++e) {
            const float dy = y2s[e * kNCT + q];
            dA1[e] = fmaf(dy, w, dA1[e]);
            acc = fmaf(dy, a1[e], acc);
          }
          if (WGRAD) row[(size_t)(cb + q) * kNH + t] += acc;
        }
      }
#pragma unroll
      for (int e = 0; e < kNTP; ++e) {
        const int p = p0 + e;
        if (p < M) {
          const int i = p / n, j = p - i * n;
          const float dz1 = a1[e] > 0.f ? dA1[e] : 0.f;
          gx += (double)dz1 * (double)(pos[2 * (o + j)] - pos[2 * (o + i)]);
          gy += (double)dz1 * (double)(pos[2 * (o + j) + 1] - pos[2 * (o + i) + 1]);
          R[(size_t)(o + j) * kNH + t] += (double)dz1;
          if (i != cur) {
            C[(size_t)(o + cur) * kNH + t] = cacc;
            cacc = 0.f;
            cur = i;
          }
          cacc += dz1;
        }
      }
    }
    C[(size_t)(o + cur) * kNH + t] = cacc;
    G[(size_t)s * 2 * kNH + 2 * t] = gx;
    G[(size_t)s * 2 * kNH + 2 * t + 1] = gy;
  }
}

// ---- finish: BatchNorm 1's backward in closed form -------------------------------------
// With yhat1[i, j, k] = uh_j + (p_j - p_i) . ah (uh = (U - mu1) rs, ah = A rs), M = n^2:
//   dbeta1 = sum_j R_j          dgamma1 = sum_j uh_j R_j + ah . G
//   dU_j = g1 (R_j - dbeta1 / n - (uh_j + (p_j - pbar) . ah) dgamma1 / n)
//   D_i  = g1 (C_i - dbeta1 / n + ((p_i - pbar) . ah) dgamma1 / n)          (sum over j of dy1)
//   dA   = g1 (G - (T + 2 Spp ah) dgamma1 / n),  T = sum_j uh_j (p_j - pbar), Spp the scatter matrix
//   dpos_m = sum_k (dU_m - D_m)[k] A_k
// Workgroup r: scenes r, r + rows, .. ; its dA / dgamma1 / dbeta1 sums stay in registers and go to
// slab row r.
__global__ void __launch_bounds__(512) pool_norm_finish_kernel(
    const float* __restrict__ U, const float* __restrict__ pos, const float* __restrict__ A,
    const float* __restrict__ gamma1, const float* __restrict__ mu1, const float* __restrict__ var1,
    const double* __restrict__ R, const float* __restrict__ C, const double* __restrict__ G,
    const int32_t* __restrict__ scene_off, int S, float eps, float* __restrict__ dU, float* __restrict__ dpos,
    float* __restrict__ slab) {
  __shared__ float2 red[64][8];
  const int k = threadIdx.x, lane = k & 63, wave = k >> 6;
  const float ax = A[2 * k], ay = A[2 * k + 1], gam = gamma1[k];
  float sAx = 0.f, sAy = 0.f, sG = 0.f, sB = 0.f;
  for (int s = blockIdx.x; s < S; s += gridDim.x) {
    const int o = scene_off[s], n = scene_off[s + 1] - o;
    if (n < 1 || n > kNMaxN) continue;
    const float2* ps = reinterpret_cast<const float2*>(pos) + o;   // (uniform addresses: the scalar cache)
    // BatchNorm's backward is a projection: its terms nearly cancel, and a small scene has a small variance
    // and a large g1 in front of the difference -- so everything up to that difference is double (O(n) work
    // per hidden unit), from R and G kept in double
    const double invn = 1.0 / (double)n;
    double mx = 0.0, my = 0.0;
    for (int j = 0; j < n; ++j) { mx += (double)ps[j].x; my += (double)ps[j].y; }
    mx *= invn; my *= invn;
    double sxx = 0.0, sxy = 0.0, syy = 0.0;
    for (int j = 0; j < n; ++j) {
      const double dx = (double)ps[j].x - mx, dy = (double)ps[j].y - my;
      sxx += dx * dx; sxy += dx * dy; syy += dy * dy;
    }
    const float mu = mu1[(size_t)s * kNH + k];
    const double rs = 1.0 / sqrt((double)var1[(size_t)s * kNH + k] + (double)eps);
    const double g1 = (double)gam * rs, ahx = (double)ax * rs, ahy = (double)ay * rs;
    const double Gx = G[(size_t)s * 2 * kNH + 2 * k], Gy = G[(size_t)s * 2 * kNH + 2 * k + 1];
    double dbd = 0.0, dgd = 0.0, txd = 0.0, tyd = 0.0;
    for (int j = 0; j < n; ++j) {
      const double uh = (double)(U[(size_t)(o + j) * kNH + k] - mu) * rs;
      const double r = R[(size_t)(o + j) * kNH + k];
      dbd += r;
      dgd += uh * r;
      txd += uh * ((double)ps[j].x - mx);
      tyd += uh * ((double)ps[j].y - my);
    }
    dgd += ahx * Gx + ahy * Gy;
    const double dgn = dgd * invn, dbn = dbd * invn;
    sAx += (float)(g1 * (Gx - dgn * (txd + 2.0 * (sxx * ahx + sxy * ahy))));
    sAy += (float)(g1 * (Gy - dgn * (tyd + 2.0 * (sxy * ahx + syy * ahy))));
    sG += (float)dgd;
    sB += (float)dbd;
    for (int jb = 0; jb < n; jb += 64) {   // dpos: blocks of 64 peds through the 8 waves' partial sums
      const int nb = min(64, n - jb);
      for (int j = jb; j < jb + nb; ++j) {
        const double uh = (double)(U[(size_t)(o + j) * kNH + k] - mu) * rs;
        const double dd = ((double)ps[j].x - mx) * ahx + ((double)ps[j].y - my) * ahy;
        const double du = g1 * (R[(size_t)(o + j) * kNH + k] - dbn - (uh + dd) * dgn);
        dU[(size_t)(o + j) * kNH + k] = (float)du;
        if (dpos) {
          const double di = g1 * ((double)C[(size_t)(o + j) * kNH + k] - dbn + dd * dgn);
          const float e = (float)(du - di);
          const float px = wave_sum(e * ax), py = wave_sum(e * ay);
          if (lane == 0) red[j - jb][wave] = make_float2(px, py);
        }
      }
      if (dpos) {
        __syncthreads();
        if (k < nb) {
          float px = 0.f, py = 0.f;
          for (int w = 0; w < 8; ++w) { px += red[k][w].x; py += red[k][w].y; }
          dpos[2 * (o + jb + k)] = px;
          dpos[2 * (o + jb + k) + 1] = py;
        }
        __syncthreads();
      }
    }
  }
  if (slab) {
    float* row = slab + (size_t)blockIdx.x * kNFinCols;
    row[2 * k] = sAx;
    row[2 * k + 1] = sAy;
    row[2 * kNH + k] = sG;
    row[3 * kNH + k] = sB;
  }
}

// rows of the dense backward's slab: more rows (scenes in flight) while the slab stays within
// 2^24 floats (64 MB), never fewer than 8 nor more than 128 -- whatever the batch
static int norm_bwd_rows(int bn) {
  long long r = (1ll << 24) / ((long long)bn * kNH + 2 * bn);
  if (r > 128) r = 128;
  if (r < 8) r = 8;
  return (int)r;
}

}  // namespace sgg

using namespace sgg;

static bool norm_sizes_ok(const char* name, int S, int B, int bn, int min_n, int max_n) {
  if (S < 0 || B < 0) {
    sgg::set_error("%s: bad sizes", name);
    return false;
  }
  if (bn < 1 || bn > SGG_POOL_BN_MAX) {
    sgg::set_error("%s: bottleneck %d outside [1, %d]", name, bn, SGG_POOL_BN_MAX);
    return false;
  }
  if (min_n < 2) {
    sgg::set_error("%s: a scene of %d ped(s): batch norm needs more than one pair row per scene", name, min_n);
    return false;
  }
  if (max_n < min_n || max_n > SGG_POOL_NORM_MAX_PEDS) {
    sgg::set_error("%s: max scene size %d outside [%d, %d]", name, max_n, min_n, SGG_POOL_NORM_MAX_PEDS);
    return false;
  }
  return true;
}

static bool norm_eps_ok(const char* name, float eps) {
  if (!(eps > 0.f) || !isfinite(eps)) {
    sgg::set_error("%s: eps %g is not a positive finite number", name, (double)eps);
    return false;
  }
  return true;
}

extern "C" int sgg_pool_norm_fwd(const float* U, const float* pos, const float* A, const float* gamma1,
                                 const float* beta1, const float* W2, const float* b2, const float* gamma2,
                                 const float* beta2, const int32_t* scene_off, int S, int B, int bn, int min_n,
                                 int max_n, float eps1, float eps2, float* Un, float* An, float* mu1, float* var1,
                                 float* mu2, float* var2, float* out, int32_t* argmax, void* stream) {
  const char* name = "sgg_pool_norm_fwd";
  SGG_CHECK_ARG(U && pos && A && gamma1 && beta1 && W2 && b2 && gamma2 && beta2 && scene_off && Un && An && mu1 &&
                    var1 && mu2 && var2 && out && argmax,
                "%s: null pointer", name);
  if (!norm_sizes_ok(name, S, B, bn, min_n, max_n)) return SGG_E_ARG;
  if (!norm_eps_ok(name, eps1) || !norm_eps_ok(name, eps2)) return SGG_E_ARG;
  if (S == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  const int nct = (bn + kNCT - 1) / kNCT;
  int gx = 4 * device_cus() / nct;
  if (gx < 1) gx = 1;
  if (gx > S) gx = S;
  hipLaunchKernelGGL(pool_norm_stats1_kernel, dim3(S < 1024 ? S : 1024), dim3(512), 0, st, U, pos, A, gamma1, beta1,
                     scene_off, S, eps1, Un, An, mu1, var1);
  hipLaunchKernelGGL(pool_norm_fwd_kernel<false>, dim3(gx, nct), dim3(512), 0, st, Un, pos, An, W2, b2, gamma2, beta2,
                     scene_off, S, bn, eps2, mu2, var2, out, argmax);
  hipLaunchKernelGGL(pool_norm_fwd_kernel<true>, dim3(gx, nct), dim3(512), 0, st, Un, pos, An, W2, b2, gamma2, beta2,
                     scene_off, S, bn, eps2, mu2, var2, out, argmax);
  SGG_RETURN_LAUNCH(name);
}

extern "C" int sgg_pool_norm_running(const float* mean, const float* var, const int32_t* scene_off, int S, int C,
                                     float momentum, float* running_mean, float* running_var, void* stream) {
  const char* name = "sgg_pool_norm_running";
  SGG_CHECK_ARG(mean && var && scene_off && running_mean && running_var, "%s: null pointer", name);
  SGG_CHECK_ARG(S >= 0 && C >= 1, "%s: bad sizes", name);
  SGG_CHECK_ARG(momentum >= 0.f && momentum <= 1.f, "%s: momentum %g outside [0, 1]", name, (double)momentum);
  if (S == 0) return 0;
  hipLaunchKernelGGL(pool_norm_running_kernel, dim3((C + 255) / 256), dim3(256), 0, (hipStream_t)stream, mean, var,
                     scene_off, S, C, momentum, running_mean, running_var);
  SGG_RETURN_LAUNCH(name);
}

extern "C" int sgg_pool_norm_bwd_rows(int bn) {
  SGG_CHECK_ARG(bn >= 1 && bn <= SGG_POOL_BN_MAX, "sgg_pool_norm_bwd_rows: bottleneck %d outside [1, %d]", bn,
                SGG_POOL_BN_MAX);
  return norm_bwd_rows(bn);
}

// [R (B x 512 doubles) | G (S x 1024 doubles) | dense slab rows x (bn 512 + 2 bn) | finish slab 32 x 2048 |
//  C (B x 512)]: the slabs start at float sgg_pool_norm_bwd_slab_offset(S, B)
extern "C" long long sgg_pool_norm_bwd_ws_floats(int S, int B, int bn) {
  if (S < 0 || B < 0 || bn < 1 || bn > SGG_POOL_BN_MAX) {
    sgg::set_error("sgg_pool_norm_bwd_ws_floats: bad sizes");
    return SGG_E_ARG;
  }
  return (long long)norm_bwd_rows(bn) * ((long long)bn * kNH + 2 * bn) + (long long)kNFinRows * kNFinCols +
         3ll * B * kNH + 4ll * S * kNH;
}

extern "C" long long sgg_pool_norm_bwd_slab_offset(int S, int B) {
  if (S < 0 || B < 0) {
    sgg::set_error("sgg_pool_norm_bwd_slab_offset: bad sizes");
    return SGG_E_ARG;
  }
  return 2ll * B * kNH + 4ll * S * kNH;
}

extern "C" int sgg_pool_norm_bwd(const float* U, const float* pos, const float* A, const float* gamma1,
                                 const float* W2, const float* b2, const float* gamma2, const float* beta2,
                                 const float* Un, const float* An, const float* mu1, const float* var1,
                                 const float* mu2, const float* var2, const float* out, const int32_t* argmax,
                                 const float* dout, const int32_t* scene_off, int S, int B, int bn, int min_n,
                                 int max_n, float eps1, float eps2, int wgrad, float* dU, float* dpos, float* ws,
                                 size_t ws_floats, void* stream) {
  const char* name = "sgg_pool_norm_bwd";
  SGG_CHECK_ARG(U && pos && A && gamma1 && W2 && b2 && gamma2 && beta2 && Un && An && mu1 && var1 && mu2 && var2 &&
                    out && argmax && dout && scene_off && dU && ws,
                "%s: null pointer", name);
  if (!norm_sizes_ok(name, S, B, bn, min_n, max_n)) return SGG_E_ARG;
  if (!norm_eps_ok(name, eps1) || !norm_eps_ok(name, eps2)) return SGG_E_ARG;
  const long long need = sgg_pool_norm_bwd_ws_floats(S, B, bn);
  SGG_CHECK_ARG((long long)ws_floats >= need, "%s: workspace of %zu floats, sgg_pool_norm_bwd_ws_floats asks for %lld",
                name, ws_floats, need);
  if (S == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  const int rows = norm_bwd_rows(bn);
  SGG_CHECK_ARG(((uintptr_t)ws & 7) == 0, "%s: workspace not 8-byte aligned", name);
  double* R = reinterpret_cast<double*>(ws);
  double* G = R + (size_t)B * kNH;
  float* slab = ws + (size_t)sgg_pool_norm_bwd_slab_offset(S, B);
  float* fin = slab + (size_t)rows * ((size_t)bn * kNH + 2 * bn);
  float* C = fin + (size_t)kNFinRows * kNFinCols;
  if (wgrad)
    hipLaunchKernelGGL(pool_norm_bwd_kernel<true>, dim3(rows), dim3(512), 0, st, Un, pos, An, W2, b2, gamma2, beta2,
                       mu2, var2, out, argmax, dout, scene_off, S, bn, eps2, slab, R, C, G);
  else
    hipLaunchKernelGGL(pool_norm_bwd_kernel<false>, dim3(rows), dim3(512), 0, st, Un, pos, An, W2, b2, gamma2, beta2,
                       mu2, var2, out, argmax, dout, scene_off, S, bn, eps2, slab, R, C, G);
  {
    hipError_t e_ = hipGetLastError();
    if (e_ != hipSuccess) {
      sgg::set_error("%s: launch failed: %s", name, hipGetErrorString(e_));
      return (int)e_;
    }
  }
  hipLaunchKernelGGL(pool_norm_finish_kernel, dim3(kNFinRows), dim3(512), 0, st, U, pos, A, gamma1, mu1, var1, R, C, G,
                     scene_off, S, eps1, dU, dpos, wgrad ? fin : nullptr);
  SGG_RETURN_LAUNCH(name);
}
