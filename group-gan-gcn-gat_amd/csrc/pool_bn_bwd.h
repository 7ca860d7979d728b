// The backward kernels of pool_bn.hip, included twice (no include guard): with
// SGG_POOL_DROP 0 this text is pool_bwd_bn_du_kernel<WGRAD> / pool_bwd_bn_dw_kernel,
// with SGG_POOL_DROP 1 pool_bwd_bn_du_drop_kernel<WGRAD> / pool_bwd_bn_dw_drop_kernel
// (sgg_pool_bwd_bn_drop), which take the dropout arguments (DropArgs) as one more
// parameter.  As a shared device function the kernels without dropout compile to
// other instruction streams (csrc/gat_kernels.h has the same form for that reason).
// The dropout forms: the output gate is dout * scale where out > 0 -- out > 0
// implies that the output mask kept the pair, so that mask is not regenerated --
// and the recomputed hidden unit k of a selected pair (i, j = argmax[i, c])
// carries the hidden mask's factor m1(i, j, k) (pool_drop.h).  m1 does not depend
// on c: its keep bits over the i any column selected are formed once per (j, i
// tile), one Philox call per such pair and thread.
#undef SGG_POOL_BN_DU_KERNEL
#undef SGG_POOL_BN_DW_KERNEL
#undef SGG_POOL_DROP_PARAM
#undef SGG_POOL_BIT
#if SGG_POOL_DROP
#define SGG_POOL_BIT(i) , i   // the pair's bit in the keep mask, one more argument of the dropout form's `entry`
#define SGG_POOL_BN_DU_KERNEL pool_bwd_bn_du_drop_kernel
#define SGG_POOL_BN_DW_KERNEL pool_bwd_bn_dw_drop_kernel
#define SGG_POOL_DROP_PARAM , const DropArgs drop
#else
#define SGG_POOL_BN_DU_KERNEL pool_bwd_bn_du_kernel
#define SGG_POOL_BN_DW_KERNEL pool_bwd_bn_dw_kernel
#define SGG_POOL_DROP_PARAM
#define SGG_POOL_BIT(i)
#endif

template <bool WGRAD>
__global__ void __launch_bounds__(512) SGG_POOL_BN_DU_KERNEL(
    const float* __restrict__ U, const float* __restrict__ pos, const float* __restrict__ A,
    const float* __restrict__ W2 /* bn x 512 */, const float* __restrict__ out,
    const int32_t* __restrict__ argmax, const float* __restrict__ dout, const int32_t* __restrict__ scene_off,
    int S, int jq, int bn, float* __restrict__ dU, float* __restrict__ dAp /* grid x 1024 */ SGG_POOL_DROP_PARAM) {
  constexpr int BN = kBT;
#if SGG_POOL_DROP
  const PoolDropKey dk = pool_drop_key(drop);
#endif
  __shared__ unsigned long long msk[kBJR * BN];   // (j - j0, c) -> set of i of the tile
  __shared__ float gs[64 * BN];                   // masked dout (i, c) of the tile
  __shared__ float2 ps[SGG_POOL_WIDE_MAX_PEDS];
  __shared__ float Us[kBJR * kHid];               // rows j0 .. j1 of U
  __shared__ float dUs[kBJR * kHid];              // their gradient, summed over column and i tiles
  const int k = threadIdx.x;   // hidden unit, blockDim.x == 512
  const int nct = (bn + BN - 1) / BN;
  float w2[BN];
  int have = -1;               // the column tile whose W2 rows sit in w2
  const float a0 = A[2 * k], a1 = A[2 * k + 1];
  float dA0 = 0.f, dA1 = 0.f;
  for (int un = blockIdx.x; un < S * jq; un += gridDim.x) {
    const int s = un / jq, jp = un - s * jq;
    const int o = scene_off[s];
    const int n = scene_off[s + 1] - o;
    const int j0 = (int)(((long long)n * jp) / jq), j1 = (int)(((long long)n * (jp + 1)) / jq);
    if (j1 <= j0) continue;   // an empty range (n < jq), uniform over the workgroup
    const int nr = j1 - j0;   // <= kBJR (host: jq >= ceil(max_n / kBJR))
    {
      const float* Ur = U + (size_t)(o + j0) * kHid + k;
#pragma unroll 4
      for (int r = 0; r < nr; ++r) {
        Us[r * kHid + k] = Ur[(size_t)r * kHid];
        dUs[r * kHid + k] = 0.f;
      }
    }
    for (int q = k; q < n; q += kHid) ps[q] = make_float2(pos[2 * (o + q)], pos[2 * (o + q) + 1]);
    for (int ct = 0; ct < nct; ++ct) {
      const int cb = ct * BN;
      const int nc = min(BN, bn - cb);
      if (ct != have) {
#pragma unroll
        for (int c = 0; c < BN; ++c) w2[c] = c < nc ? W2[(size_t)(cb + c) * kHid + k] : 0.f;
        have = ct;
      }
      for (int t0 = 0; t0 < n; t0 += 64) {
        const int ni = min(64, n - t0);
        const int ne = ni * BN;
        for (int e = k; e < kBJR * BN; e += kHid) msk[e] = 0ull;
        __syncthreads();   // masks cleared before the ORs; the unit's ps written
#pragma unroll 2
        for (int e = k; e < ne; e += kHid) {
          const int i = e / BN, c = e - i * BN;
          if (c < nc) {
            const size_t ge = (size_t)(o + t0 + i) * bn + cb + c;
            const float ov = out[ge], dv = dout[ge];
            const int jl = argmax[ge] - o - j0;
#if SGG_POOL_DROP
            const float g = ov > 0.f ? __fmul_rn(dv, dk.scale) : 0.f;
#else
            const float g = ov > 0.f ? dv : 0.f;
#endif
            gs[e] = g;
            if (g != 0.f && jl >= 0 && jl < nr) atomicOr(&msk[jl * BN + c], 1ull << i);
          }
        }
        __syncthreads();
        for (int r = 0; r < nr; ++r) {
          const float u = Us[r * kHid + k];
          const float2 pj = ps[j0 + r];
          float du = dUs[r * kHid + k];
#if SGG_POOL_DROP
          // the hidden mask's keep bits of (i, j0 + r, k) for the i any column selected, once per (j, i tile):
          // the mask does not depend on the column
          unsigned long long need = 0ull;
          for (int c = 0; c < BN; ++c) need |= msk[r * BN + c];
          const unsigned long long kp = pool_drop_keep_bits(dk, wave_uniform(need), (uint32_t)(o + t0),
                                                            (uint32_t)(j0 + r), (uint32_t)k);
#endif
          constexpr int CB = 16;
          unsigned long long mrow[CB];
#pragma unroll
          for (int c = 0; c < BN; ++c) {
            if (c % CB == 0) {
#pragma unroll
              for (int cc = 0; cc < CB; ++cc) mrow[cc] = msk[r * BN + c + cc];
            }
            const unsigned long long mv = mrow[c % CB];
            const unsigned mhi = (unsigned)__builtin_amdgcn_readfirstlane((unsigned)(mv >> 32));
            const unsigned mlo = (unsigned)__builtin_amdgcn_readfirstlane((unsigned)mv);
            unsigned long long m = ((unsigned long long)mhi << 32) | (unsigned long long)mlo;
            // two set bits per trip, taken in ascending i one at a time (pool_bwd_wide_kernel)
#if SGG_POOL_DROP
            auto entry = [&](float g, float2 pi, int i) {
              const float rx = pj.x - pi.x, ry = pj.y - pi.y;
              const float pre = fmaf(a1, ry, fmaf(a0, rx, u));
              const float gm = pre > 0.f && ((kp >> i) & 1ull) ? __fmul_rn(g, dk.scale) : 0.f;
#else
            auto entry = [&](float g, float2 pi) {
              const float rx = pj.x - pi.x, ry = pj.y - pi.y;
              const float pre = fmaf(a1, ry, fmaf(a0, rx, u));
              const float gm = pre > 0.f ? g : 0.f;
#endif
              const float d = gm * w2[c];
              du += d;
              if (WGRAD) {
                dA0 = fmaf(d, rx, dA0);
                dA1 = fmaf(d, ry, dA1);
              }
            };
            while (m) {
              const int i = __builtin_ctzll(m);
              m &= m - 1;
              const bool two = m != 0;   // uniform
              const int i2 = two ? __builtin_ctzll(m) : i;
              if (two) m &= m - 1;
              const float g = gs[i * BN + c], g2 = gs[i2 * BN + c];
              const float2 pi = ps[t0 + i], pi2 = ps[t0 + i2];
              entry(g, pi SGG_POOL_BIT(i));
              if (two) entry(g2, pi2 SGG_POOL_BIT(i2));
            }
          }
          dUs[r * kHid + k] = du;
        }
        __syncthreads();   // the walk is done: msk / gs (and, after the last tile, ps) may be rewritten
      }
    }
    for (int r = 0; r < nr; ++r) dU[(size_t)(o + j0 + r) * kHid + k] = dUs[r * kHid + k];
  }
  if (WGRAD) {
    dAp[(size_t)blockIdx.x * 2 * kHid + 2 * k] = dA0;
    dAp[(size_t)blockIdx.x * 2 * kHid + 2 * k + 1] = dA1;
  }
}

__global__ void __launch_bounds__(512) SGG_POOL_BN_DW_KERNEL(
    const float* __restrict__ U, const float* __restrict__ pos, const float* __restrict__ A,
    const float* __restrict__ out, const int32_t* __restrict__ argmax, const float* __restrict__ dout,
    const int32_t* __restrict__ scene_off, int S, int jq, int bn, const float* __restrict__ dAp, int ndA,
    float* __restrict__ part /* kBRows x (bn*512 + 1024 + bn) */ SGG_POOL_DROP_PARAM) {
  constexpr int CG = kBCG;
#if SGG_POOL_DROP
  const PoolDropKey dk = pool_drop_key(drop);
#endif
  __shared__ unsigned long long msk[kBJR * CG];
  __shared__ float gs[64 * CG];
  __shared__ float2 ps[SGG_POOL_WIDE_MAX_PEDS];
  __shared__ float Us[kBJR * kHid];
  const int k = threadIdx.x;   // hidden unit, blockDim.x == 512
  const int cb = (int)blockIdx.x * CG;
  const int nc = min(CG, bn - cb);   // >= 1: grid.x = ceil(bn / CG)
  const int row = (int)blockIdx.y;
  float dw2[CG];
#pragma unroll
  for (int c = 0; c < CG; ++c) dw2[c] = 0.f;
  const float a0 = A[2 * k], a1 = A[2 * k + 1];
  float db2 = 0.f;
  for (int un = row; un < S * jq; un += kBRows) {
    const int s = un / jq, jp = un - s * jq;
    const int o = scene_off[s];
    const int n = scene_off[s + 1] - o;
    const int j0 = (int)(((long long)n * jp) / jq), j1 = (int)(((long long)n * (jp + 1)) / jq);
    if (j1 <= j0) continue;
    const int nr = j1 - j0;
    {
      const float* Ur = U + (size_t)(o + j0) * kHid + k;
#pragma unroll 4
      for (int r = 0; r < nr; ++r) Us[r * kHid + k] = Ur[(size_t)r * kHid];
    }
    for (int q = k; q < n; q += kHid) ps[q] = make_float2(pos[2 * (o + q)], pos[2 * (o + q) + 1]);
    for (int t0 = 0; t0 < n; t0 += 64) {
      const int ni = min(64, n - t0);
      const int ne = ni * CG;
      for (int e = k; e < kBJR * CG; e += kHid) msk[e] = 0ull;
      __syncthreads();
      for (int e = k; e < ne; e += kHid) {
        const int i = e / CG, c = e - i * CG;
        float g = 0.f;
        if (c < nc) {
          const size_t ge = (size_t)(o + t0 + i) * bn + cb + c;
          const float ov = out[ge], dv = dout[ge];
          const int jl = argmax[ge] - o - j0;
#if SGG_POOL_DROP
          g = ov > 0.f ? __fmul_rn(dv, dk.scale) : 0.f;
#else
          g = ov > 0.f ? dv : 0.f;
#endif
          if (g != 0.f && jl >= 0 && jl < nr) atomicOr(&msk[jl * CG + c], 1ull << i);
        }
        gs[e] = g;
      }
      __syncthreads();
      // db2 once per scene: by the unit of the scene's last (never empty) range
      if (jp == jq - 1 && k < nc)
        for (int i = 0; i < ni; ++i) db2 += gs[i * CG + k];
      for (int r = 0; r < nr; ++r) {
        const float u = Us[r * kHid + k];
        const float2 pj = ps[j0 + r];
        unsigned long long mrow[CG];
#pragma unroll
        for (int c = 0; c < CG; ++c) mrow[c] = msk[r * CG + c];
#if SGG_POOL_DROP
        unsigned long long need = 0ull;   // the hidden mask's keep bits, as in the dU kernel
#pragma unroll
        for (int c = 0; c < CG; ++c) need |= mrow[c];
        const unsigned long long kp = pool_drop_keep_bits(dk, wave_uniform(need), (uint32_t)(o + t0),
                                                          (uint32_t)(j0 + r), (uint32_t)k);
#endif
#pragma unroll
        for (int c = 0; c < CG; ++c) {
          const unsigned mhi = (unsigned)__builtin_amdgcn_readfirstlane((unsigned)(mrow[c] >> 32));
          const unsigned mlo = (unsigned)__builtin_amdgcn_readfirstlane((unsigned)mrow[c]);
          unsigned long long m = ((unsigned long long)mhi << 32) | (unsigned long long)mlo;
          while (m) {   // ascending i
            const int i = __builtin_ctzll(m);
            m &= m - 1;
            const float g = gs[i * CG + c];
            const float2 pi = ps[t0 + i];
            const float rx = pj.x - pi.x, ry = pj.y - pi.y;
            const float pre = fmaf(a1, ry, fmaf(a0, rx, u));
            const float gm = pre > 0.f ? g : 0.f;
#if SGG_POOL_DROP
            dw2[c] = fmaf(gm, (kp >> i) & 1ull ? __fmul_rn(pre, dk.scale) : 0.f, dw2[c]);   // gm (m1 pre)
#else
            dw2[c] = fmaf(gm, pre, dw2[c]);
#endif
          }
        }
      }
      __syncthreads();
    }
  }
  // row `row` of the slab [dW2 (bn x 512) | dA (512 x 2) | db2 (bn)]: this workgroup's columns
  float* prow = part + (size_t)row * ((size_t)bn * kHid + 2 * kHid + bn);
#pragma unroll
  for (int c = 0; c < CG; ++c)
    if (c < nc) prow[(size_t)(cb + c) * kHid + k] = dw2[c];
  if (k < nc) prow[(size_t)bn * kHid + 2 * kHid + cb + k] = db2;
  if (blockIdx.x == 0) {
    float s0 = 0.f, s1 = 0.f;
    for (int g = row; g < ndA; g += kBRows) {
      s0 += dAp[(size_t)g * 2 * kHid + 2 * k];
      s1 += dAp[(size_t)g * 2 * kHid + 2 * k + 1];
    }
    prow[(size_t)bn * kHid + 2 * k] = s0;
    prow[(size_t)bn * kHid + 2 * k + 1] = s1;
  }
}
