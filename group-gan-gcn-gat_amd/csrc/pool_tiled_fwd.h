// The tiled pooling forward (pool_wide.hip, pool_bn.hip): one body for both kernel families.
#pragma once
#include "sgg_common.h"
#include "pool_common.h"
#include "pool_drop.h"

namespace sgg {

// Work unit = a chunk of whole i-rows [i0, i1) of one scene (sgg_pool_plan_wide),
// so max_j still completes inside one workgroup (LDS atomics only).  The
// workgroup walks the scene's j in tiles of <= 64 peds and, inside a tile, its
// rows x nj pairs (j fastest) in passes of its pair capacity (4 waves x GPW
// groups x 16 pairs).  A pass is pool_fwd_kernel's chunk body: the 512 hidden
// units in k-tiles of 64 staged in LDS (the j-tile's U rows, W2^T tile, A
// tile), k-steps of 4 through v_mfma_f32_16x16x4_f32, one hidden value per lane
// and group (2 FMA + max), bias then ReLU -- a pair's value does not depend on
// the tiling, so it is bitwise pool_fwd_kernel's.  The keys (value bits << 32 |
// ~j, j scene-local) live in LDS across all tiles and passes and are written
// out once.  The next k-tile -- of this pass, or the first of the next pass /
// j-tile -- is register-staged while the current one computes.
constexpr int kWKT = 64;           // hidden units per LDS k-tile
constexpr int kWKTP = kWKT + 2;    // U tile row stride: (2j + k) mod 32 -> conflict-free b32 reads
constexpr int kWJT = 64;           // peds per j-tile
constexpr int kWideWaves = 4;

// The forward's body, shared by pool_fwd_wide_kernel<BN, GPW> (RT = false: all BN columns, row stride BN,
// everything below a compile-time constant) and pool_fwd_bn_kernel (pool_bn.hip; RT = true, BN = 64: the
// column tile [cb, cb + ncol) of a W2 / b2 / out / argmax with the runtime row stride bn_rt -- columns
// >= ncol of the tile have their W2 rows staged as 0 and are neither max-ed nor stored).
// DROP (pool_fwd_bn_drop_kernel): the hidden value is m1 * relu(..), the epilogue value m2 * relu(..), m the
// scaled masks of pool_drop.h -- one Philox call per group and four k-steps for m1 (the lane's hidden units
// k0 + 16 q + 4 s + kq, s = 0..3, are the call's four words), one per output element for m2.  Neither mask
// sees cb, the j-tile or the pass: every column tile recomputes the same hidden mask.
template <int BN, int GPW, bool RT, bool DROP = false>
__device__ __forceinline__ void pool_fwd_tiled_body(
    const float* __restrict__ U, const float* __restrict__ pos, const float* __restrict__ A,
    const float* __restrict__ W2 /* stride x 512 */, const float* __restrict__ b2,
    const int32_t* __restrict__ scene_off, const int4* __restrict__ chunks, int nch, float* __restrict__ out,
    int32_t* __restrict__ argmax, int cb_rt, int bn_rt, const DropArgs& drop = DropArgs{}) {
  PoolDropKey dk{};
  if constexpr (DROP) dk = pool_drop_key(drop);
  const int cb = RT ? cb_rt : 0;                       // first column of the tile
  const int stride = RT ? bn_rt : BN;                  // row stride of W2 / out / argmax, length of b2
  const int ncol = RT ? min(BN, bn_rt - cb_rt) : BN;   // live columns of the tile
  using C = PoolCfg<BN>;
  constexpr int NT = C::NT, BNP = C::BNP;
  constexpr int P = 16 * kWideWaves * GPW;   // pairs of one pass
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* Us = reinterpret_cast<float*>(smem);                              // kWJT x kWKTP
  float* W2s = Us + kWJT * kWKTP;                                          // kWKT x BNP
  float* As = W2s + kWKT * BNP;                                            // kWKT x 2
  float2* ps = reinterpret_cast<float2*>(As + 2 * kWKT);                   // scene positions (<= 1024)
  unsigned long long* keys = reinterpret_cast<unsigned long long*>(ps + SGG_POOL_WIDE_MAX_PEDS);  // rows x BN
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int c16 = lane & 15, kq = lane >> 4;
  float bv[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) bv[t] = b2[min(cb + 16 * t + c16, stride - 1)];

  // XCD-aware chunk order (pool_fwd_kernel): the grid is a multiple of 8
  const int gstride = (int)gridDim.x;
  const int xb = ((int)blockIdx.x & 7) * (gstride >> 3) + ((int)blockIdx.x >> 3);
  for (int ch = xb; ch < nch; ch += gstride) {
    const int4 cd = chunks[ch];
    const int s = cd.x, i0 = cd.y, i1 = cd.z;
    if (i1 <= i0) continue;
    const int o = scene_off[s];
    const int n = scene_off[s + 1] - o;
    const int rows = i1 - i0;
    const int ntiles = (n + kWJT - 1) / kWJT;

    for (int q = threadIdx.x; q < n; q += blockDim.x) ps[q] = make_float2(pos[2 * (o + q)], pos[2 * (o + q) + 1]);
    for (int q = threadIdx.x; q < rows * BN; q += blockDim.x) keys[q] = 0ull;

    constexpr int kUQ = (kWJT * (kWKT / 4) + 255) / 256;   // float4 of U per thread
    constexpr int kWQ = (kWKT * BNP + 255) / 256;          // W2^T floats per thread
    float4 ureg[kUQ];
    float wreg[kWQ];
    float areg = 0.f;
    int nj_ld = 0;   // rows of the register-staged U tile
    auto load_tile = [&](int jb, int nj, int k0) {
      nj_ld = nj;
#pragma unroll
      for (int e = 0; e < kUQ; ++e) {
        const int q = threadIdx.x + 256 * e;
        const int r = q / (kWKT / 4), c4 = q - r * (kWKT / 4);
        if (r < nj) ureg[e] = *reinterpret_cast<const float4*>(U + (size_t)(o + jb + r) * kHidden + k0 + 4 * c4);
      }
#pragma unroll
      for (int e = 0; e < kWQ; ++e) {   // W2 (BN x 512, nn.Linear layout), read transposed
        const int q = threadIdx.x + 256 * e;
        const int kk = q / BNP, cc = q - kk * BNP;
        wreg[e] = (kk < kWKT && cc < ncol) ? W2[(size_t)(cb + cc) * kHidden + k0 + kk] : 0.f;
      }
      if (threadIdx.x < 2 * kWKT) areg = A[2 * k0 + threadIdx.x];
    };
    auto store_tile = [&]() {
#pragma unroll
      for (int e = 0; e < kUQ; ++e) {
        const int q = threadIdx.x + 256 * e;
        const int r = q / (kWKT / 4), c4 = q - r * (kWKT / 4);
        if (r < nj_ld) {
          float* d = Us + r * kWKTP + 4 * c4;
          d[0] = ureg[e].x; d[1] = ureg[e].y; d[2] = ureg[e].z; d[3] = ureg[e].w;
        }
      }
#pragma unroll
      for (int e = 0; e < kWQ; ++e) {
        const int q = threadIdx.x + 256 * e;
        if (q < kWKT * BNP) W2s[q] = wreg[e];
      }
      if (threadIdx.x < 2 * kWKT) As[threadIdx.x] = areg;
    };

    load_tile(0, min(kWJT, n), 0);
    __syncthreads();  // ps / keys init visible; the previous chunk's readers done
    store_tile();
    __syncthreads();
    for (int jt = 0; jt < ntiles; ++jt) {
      const int jb = jt * kWJT;
      const int nj = min(kWJT, n - jb);
      const int npairs = rows * nj;
      const int npass = (npairs + P - 1) / P;
      for (int pa = 0; pa < npass; ++pa) {
        // what follows this pass: another pass of the tile, the next tile, or nothing
        const bool more = pa + 1 < npass || jt + 1 < ntiles;
        const int jb_n = pa + 1 < npass ? jb : jb + kWJT;
        const int nj_n = min(kWJT, n - jb_n);

        // per-lane A-row pair of each group (padding pairs -> the tile's first j, r = 0)
        int uoff[GPW];
        float rx[GPW], ry[GPW];
        floatx4 acc[GPW][NT];
        uint32_t di[GPW], dj[GPW];   // DROP: the lane's pair (global i, scene-local j << 8 | kq) of each group
#pragma unroll
        for (int g = 0; g < GPW; ++g) {
          const int p = pa * P + (wave * GPW + g) * 16 + c16;
          int il = 0, jl = 0;
          if (p < npairs) { il = p / nj; jl = p - il * nj; }
          uoff[g] = jl * kWKTP + kq;
          if constexpr (DROP) {
            di[g] = (uint32_t)(o + i0 + il);
            dj[g] = ((uint32_t)(jb + jl) << 8) | (uint32_t)kq;
          }
          const float2 pj = ps[jb + jl], pi = ps[i0 + il];
          rx[g] = p < npairs ? pj.x - pi.x : 0.f;
          ry[g] = p < npairs ? pj.y - pi.y : 0.f;
#pragma unroll
          for (int t = 0; t < NT; ++t) acc[g][t] = floatx4{0.f, 0.f, 0.f, 0.f};
        }

        for (int k0 = 0; k0 < kHidden; k0 += kWKT) {
          const bool last_k = k0 + kWKT >= kHidden;
          if (!last_k) load_tile(jb, nj, k0 + kWKT);
          else if (more) load_tile(jb_n, nj_n, 0);
          float b[NT], u[GPW];
          float2 a;
#pragma unroll
          for (int t = 0; t < NT; ++t) b[t] = W2s[kq * BNP + 16 * t + c16];
          a = *reinterpret_cast<const float2*>(As + 2 * kq);
#pragma unroll
          for (int g = 0; g < GPW; ++g) u[g] = Us[uoff[g]];
          if constexpr (DROP) {
            // the k-steps below, four at a time under one mask call per group: its words 0..3 are the lane's
            // hidden units k0 + 16 q4 + 4 sq + kq
            for (int q4 = 0; q4 < kWKT / 16; ++q4) {
              Philox4 x[GPW];
#pragma unroll
              for (int g = 0; g < GPW; ++g)
                x[g] = philox4x32_10(di[g], dj[g] | (uint32_t)(((k0 >> 4) + q4) << 2),
                                     (uint32_t)SGG_POOL_DROP_SITE_HIDDEN << 8, dk.c3, dk.k0, dk.k1);
#pragma unroll
              for (int sq = 0; sq < 4; ++sq) {
                const int s4 = 4 * q4 + sq;
                float h[GPW], bc[NT];
#pragma unroll
                for (int g = 0; g < GPW; ++g)
                  h[g] = __fmul_rn(fmaxf(fmaf(a.y, ry[g], fmaf(a.x, rx[g], u[g])), 0.f), pool_drop_mul(dk, x[g].w[sq]));
#pragma unroll
                for (int t = 0; t < NT; ++t) bc[t] = b[t];
                if (s4 + 1 < kWKT / 4) {
                  const int kn = 4 * (s4 + 1);
#pragma unroll
                  for (int t = 0; t < NT; ++t) b[t] = W2s[(kn + kq) * BNP + 16 * t + c16];
                  a = *reinterpret_cast<const float2*>(As + 2 * (kn + kq));
#pragma unroll
                  for (int g = 0; g < GPW; ++g) u[g] = Us[uoff[g] + kn];
                }
#pragma unroll
                for (int g = 0; g < GPW; ++g)
#pragma unroll
                  for (int t = 0; t < NT; ++t)
                    acc[g][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(h[g], bc[t], acc[g][t], 0, 0, 0);
              }
            }
          } else {
#pragma unroll 2
          for (int s4 = 0; s4 < kWKT / 4; ++s4) {
            float h[GPW], bc[NT];
#pragma unroll
            for (int g = 0; g < GPW; ++g) h[g] = fmaxf(fmaf(a.y, ry[g], fmaf(a.x, rx[g], u[g])), 0.f);
#pragma unroll
            for (int t = 0; t < NT; ++t) bc[t] = b[t];
            if (s4 + 1 < kWKT / 4) {  // prefetch the next k-step's operands
              const int kn = 4 * (s4 + 1);
#pragma unroll
              for (int t = 0; t < NT; ++t) b[t] = W2s[(kn + kq) * BNP + 16 * t + c16];
              a = *reinterpret_cast<const float2*>(As + 2 * (kn + kq));
#pragma unroll
              for (int g = 0; g < GPW; ++g) u[g] = Us[uoff[g] + kn];
            }
#pragma unroll
            for (int g = 0; g < GPW; ++g)
#pragma unroll
              for (int t = 0; t < NT; ++t)
                acc[g][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(h[g], bc[t], acc[g][t], 0, 0, 0);
          }
          }
          __syncthreads();  // tile consumed
          if (!last_k || more) {
            store_tile();
            __syncthreads();
          }
        }

        // DROP: the output mask's keep bits of the lane's (g, r, t) elements, by a loop that stays rolled (the
        // epilogue below must unroll for acc's static indices; with the mask calls inside it does not)
        unsigned long long kb = 0ull;
        if constexpr (DROP) {
          static_assert(4 * GPW * NT <= 64, "keep bits of one pass in 64 bits");
#pragma unroll 1
          for (int gr = 0; gr < 4 * GPW; ++gr) {
            const int p = pa * P + (wave * GPW + (gr >> 2)) * 16 + kq * 4 + (gr & 3);
            if (p < npairs) {
              const int il = p / nj, j = jb + (p - il * nj);
#pragma unroll
              for (int t = 0; t < NT; ++t)
                kb |= (unsigned long long)pool_drop_keep(dk, SGG_POOL_DROP_SITE_OUT, (uint32_t)(o + i0 + il), (uint32_t)j,
                                                         (uint32_t)(cb + 16 * t + c16))
                      << (gr * NT + t);
            }
          }
        }

        // epilogue: bias, ReLU, max over j (LDS atomic max on (bits << 32 | ~j))
#pragma unroll
        for (int g = 0; g < GPW; ++g) {
          const int grp = wave * GPW + g;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int p = pa * P + grp * 16 + kq * 4 + r;
            if (p < npairs) {
              const int il = p / nj, j = jb + (p - il * nj);
              const unsigned long long jkey = 0xFFFFFFFFull - (unsigned long long)j;
#pragma unroll
              for (int t = 0; t < NT; ++t) {
                const int cc = 16 * t + c16;
                if (cc < ncol) {
                  float v = acc[g][t][r] + bv[t];
                  v = v > 0.f ? v : 0.f;
                  if constexpr (DROP) v = (kb >> ((4 * g + r) * NT + t)) & 1ull ? __fmul_rn(v, dk.scale) : 0.f;
                  atomicMax(&keys[il * BN + cc], ((unsigned long long)__float_as_uint(v) << 32) | jkey);
                }
              }
            }
          }
        }
      }
    }
    __syncthreads();
    for (int q = threadIdx.x; q < rows * BN; q += blockDim.x) {
      size_t oi = (size_t)(o + i0) * BN + q;
      if (RT) {
        const int il = q / BN, cc = q - il * BN;
        if (cc >= ncol) continue;
        oi = (size_t)(o + i0 + il) * stride + cb + cc;
      }
      const unsigned long long key = keys[q];
      out[oi] = __uint_as_float((unsigned)(key >> 32));
      argmax[oi] = o + (int)(0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull));
    }
    __syncthreads();
  }
}

// dynamic LDS of the body at chunks of up to max_rows rows
template <int BN>
static inline size_t pool_fwd_tiled_lds(int max_rows) {
  using C = PoolCfg<BN>;
  return sizeof(float) * ((size_t)kWJT * kWKTP + (size_t)kWKT * C::BNP + 2 * kWKT) +
         sizeof(float2) * SGG_POOL_WIDE_MAX_PEDS + sizeof(unsigned long long) * (size_t)max_rows * BN;
}

}  // namespace sgg
