// Social pooling for scenes above SGG_POOL_MAX_PEDS (up to
// SGG_POOL_WIDE_MAX_PEDS) peds: the pair space tiled in j (forward) and in i
// (backward).  Same factoring, operands and results as pool.hip, whose
// kernels hold a whole scene in LDS; here nothing in LDS but the scene's
// positions (8 KiB at 1024 peds) grows with the scene.
#include <stdlib.h>
#include <string.h>

#include "sgg_common.h"
#include "pool_common.h"
#include "pool_tiled_fwd.h"

namespace sgg {

// ---- forward ------------------------------------------------------------------
// pool_tiled_fwd.h: the body shared with the column-tiled family (pool_bn.hip); here every column of the
// template width, compile-time strides.
template <int BN, int GPW>
__global__ void __launch_bounds__(256) pool_fwd_wide_kernel(
    const float* __restrict__ U, const float* __restrict__ pos, const float* __restrict__ A,
    const float* __restrict__ W2 /* BN x 512 */, const float* __restrict__ b2,
    const int32_t* __restrict__ scene_off, const int4* __restrict__ chunks, int nch, float* __restrict__ out,
    int32_t* __restrict__ argmax) {
  pool_fwd_tiled_body<BN, GPW, false>(U, pos, A, W2, b2, scene_off, chunks, nch, out, argmax, 0, BN);
}

// ---- backward -----------------------------------------------------------------
// Only (i, argmax[i, c]) carries gradient.  Work unit = (scene, j range of
// <= kWideJR peds): every scene is cut into jq ranges (floor boundaries).  The
// unit walks the scene's i in tiles of 64, ascending: per tile it loads the
// masked dout (gs) of those 64 rows and rebuilds, for its own j range only,
// the (j, c) masks over the tile's i (LDS atomic OR: order-free), then runs
// pool_bwd_kernel's per-entry chain -- thread k = hidden unit k, W2[c][k] and
// the dW2[c][k] partial in registers, the bit walk scalar, the per-entry
// operands wave-uniform LDS broadcasts.  The unit's U rows are staged in LDS
// once; dU[j, k] is carried across the tiles in the thread's own LDS column
// (a register array indexed by the running j would live in scratch, and
// unrolling j x c multiplies the code by the range) and stored once.  Every
// sum has a fixed order: ascending i within a tile, tiles ascending; each
// workgroup writes its [dW2 | dA | db2] partial to its own slab row.  db2 is
// added once per scene, by the unit of the scene's last (never empty) range.
// LDS: 24 BN + 8 K for masks / gs / positions plus 2 x kWideJR x 2 KiB for the
// U and dU rows -- independent of the scene size.
constexpr int kWideJR = 16;

template <int BN, bool WGRAD>
__global__ void __launch_bounds__(512) pool_bwd_wide_kernel(
    const float* __restrict__ U, const float* __restrict__ pos, const float* __restrict__ A,
    const float* __restrict__ W2 /* BN x 512 */, const float* __restrict__ out,
    const int32_t* __restrict__ argmax, const float* __restrict__ dout, const int32_t* __restrict__ scene_off,
    int S, int jq, float* __restrict__ dU, float* __restrict__ part) {
  __shared__ unsigned long long msk[kWideJR * BN];   // (j - j0, c) -> set of i of the tile
  __shared__ float gs[64 * BN];                      // masked dout (i, c) of the tile
  __shared__ float2 ps[SGG_POOL_WIDE_MAX_PEDS];
  __shared__ float Us[kWideJR * kHidden];            // rows j0 .. j1 of U
  __shared__ float dUs[kWideJR * kHidden];           // their gradient, summed over the tiles
  const int k = threadIdx.x;   // hidden unit, blockDim.x == 512
  float w2[BN], dw2[BN];
#pragma unroll
  for (int c = 0; c < BN; ++c) {
    w2[c] = W2[c * kHidden + k];
    dw2[c] = 0.f;
  }
  const float a0 = A[2 * k], a1 = A[2 * k + 1];
  float dA0 = 0.f, dA1 = 0.f, db2 = 0.f;
  for (int un = blockIdx.x; un < S * jq; un += gridDim.x) {
    const int s = un / jq, jp = un - s * jq;
    const int o = scene_off[s];
    const int n = scene_off[s + 1] - o;
    const int j0 = (int)(((long long)n * jp) / jq), j1 = (int)(((long long)n * (jp + 1)) / jq);
    if (j1 <= j0) continue;   // an empty range (n < jq), uniform over the workgroup
    const int nr = j1 - j0;   // <= kWideJR (host: jq >= ceil(max_n / kWideJR))
    {
      const float* Ur = U + (size_t)(o + j0) * kHidden + k;
#pragma unroll 4
      for (int r = 0; r < nr; ++r) {
        Us[r * kHidden + k] = Ur[(size_t)r * kHidden];
        dUs[r * kHidden + k] = 0.f;
      }
    }
    for (int q = k; q < n; q += kHidden) ps[q] = make_float2(pos[2 * (o + q)], pos[2 * (o + q) + 1]);
    for (int t0 = 0; t0 < n; t0 += 64) {
      const int ni = min(64, n - t0);
      const int ne = ni * BN;
      for (int e = k; e < kWideJR * BN; e += kHidden) msk[e] = 0ull;
      __syncthreads();   // masks cleared before the ORs
#pragma unroll 2
      for (int e = k; e < ne; e += kHidden) {
        const size_t ge = (size_t)(o + t0) * BN + e;
        const float ov = out[ge], dv = dout[ge];
        const int jl = argmax[ge] - o - j0;
        const float g = ov > 0.f ? dv : 0.f;
        gs[e] = g;
        if (g != 0.f && jl >= 0 && jl < nr) {
          const int i = e / BN, c = e - i * BN;
          atomicOr(&msk[jl * BN + c], 1ull << i);
        }
      }
      __syncthreads();
      if (WGRAD && jp == jq - 1 && k < BN)
        for (int i = 0; i < ni; ++i) db2 += gs[i * BN + k];
      for (int r = 0; r < nr; ++r) {
        const float u = Us[r * kHidden + k];
        const float2 pj = ps[j0 + r];
        float du = dUs[r * kHidden + k];
        constexpr int CB = BN < 16 ? BN : 16;
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
          // two set bits per trip, taken in ascending i one at a time (pool_bwd_kernel)
          auto entry = [&](float g, float2 pi) {
            const float rx = pj.x - pi.x, ry = pj.y - pi.y;
            const float pre = fmaf(a1, ry, fmaf(a0, rx, u));
            const float gm = pre > 0.f ? g : 0.f;
            const float d = gm * w2[c];
            du += d;
            if (WGRAD) {
              dw2[c] = fmaf(gm, pre, dw2[c]);
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
            entry(g, pi);
            if (two) entry(g2, pi2);
          }
        }
        dUs[r * kHidden + k] = du;
      }
      __syncthreads();   // the walk is done: msk / gs (and, after the last tile, ps) may be rewritten
    }
    for (int r = 0; r < nr; ++r) dU[(size_t)(o + j0 + r) * kHidden + k] = dUs[r * kHidden + k];
  }
  if (WGRAD) {   // this workgroup's row of the parameter-gradient slab: [dW2 (BN x 512) | dA (512 x 2) | db2 (BN)]
    float* row = part + (size_t)blockIdx.x * (BN * kHidden + 2 * kHidden + BN);
#pragma unroll
    for (int c = 0; c < BN; ++c) row[c * kHidden + k] = dw2[c];
    row[BN * kHidden + 2 * k] = dA0;
    row[BN * kHidden + 2 * k + 1] = dA1;
    if (k < BN) row[BN * kHidden + 2 * kHidden + k] = db2;
  }
}

// pair groups per wave: the resident kernel's measured caps
static int wide_gpw(int bn) { return bn > 16 ? 4 : 2; }

template <int BN, int GPW>
static int launch_fwd_wide(const float* U, const float* pos, const float* A, const float* W2, const float* b2,
                           const int32_t* off, const int32_t* chunks, int nchunks, int max_rows, float* out,
                           int32_t* am, hipStream_t st) {
  // a multiple of 8 workgroups (XCD-aware order), at most four rounds of the chip
  int grid = (nchunks + 7) & ~7;
  const int cap = 4 * ((device_cus() + 7) & ~7);
  if (grid > cap) grid = cap;
  hipLaunchKernelGGL((pool_fwd_wide_kernel<BN, GPW>), dim3(grid), dim3(256), pool_fwd_tiled_lds<BN>(max_rows), st, U, pos, A,
                     W2, b2, off, reinterpret_cast<const int4*>(chunks), nchunks, out, am);
  SGG_RETURN_LAUNCH("sgg_pool_fwd_wide");
}

// j ranges per scene of the wide backward: at least ceil(max_n / kWideJR) (a
// range fits the LDS rows), more while S x jq stays within one round of the chip
static int wide_bwd_jq(int S, int max_n) {
  if (S < 1 || max_n < 1) return 1;
  int jq = (max_n + kWideJR - 1) / kWideJR;
  const int fill = 256 / S;
  if (fill > jq) jq = fill < max_n ? fill : max_n;
  return jq < 1 ? 1 : jq;
}

template <int BN>
static int launch_bwd_wide(const float* U, const float* pos, const float* A, const float* W2, const float* out,
                           const int32_t* am, const float* dout, const int32_t* off, int S, int max_n, float* dU,
                           float* part, hipStream_t st) {
  const int grid = sgg_pool_bwd_wide_grid(S, max_n), jq = wide_bwd_jq(S, max_n);
  if (part)
    hipLaunchKernelGGL((pool_bwd_wide_kernel<BN, true>), dim3(grid), dim3(512), 0, st, U, pos, A, W2, out, am, dout,
                       off, S, jq, dU, part);
  else
    hipLaunchKernelGGL((pool_bwd_wide_kernel<BN, false>), dim3(grid), dim3(512), 0, st, U, pos, A, W2, out, am, dout,
                       off, S, jq, dU, part);
  SGG_RETURN_LAUNCH("sgg_pool_bwd_wide");
}

}  // namespace sgg

using namespace sgg;

static bool wide_bn_ok(int bn) { return bn == 8 || bn == 16 || bn == 32 || bn == 48 || bn == 64; }

// host helper of sgg_pool_plan_wide / sgg_pool_plan_bn (arguments checked by
// the caller): chunks of whole i-rows, at most rmax rows each -- rmax the
// largest of 64, 32, .. gpw that still yields >= target_chunks chunks (64
// bounds the keys in LDS; gpw rows x a full 64-ped j-tile fill one pass) --
// rows spread evenly over a scene's chunks
int sgg::pool_plan_rows(const char* name, const int32_t* host_scene_off, int S, int gpw, int target_chunks,
                        int32_t* chunks, int cap, int* max_rows, int* gpw_out) {
  for (int s = 0; s < S; ++s) {
    const int n = host_scene_off[s + 1] - host_scene_off[s];
    if (n < 0 || n > SGG_POOL_WIDE_MAX_PEDS) {
      sgg::set_error("%s: scene %d has %d peds, outside [0, %d]", name, s, n, SGG_POOL_WIDE_MAX_PEDS);
      return SGG_E_ARG;
    }
  }
  int rmax = 64;
  for (; rmax > gpw; rmax >>= 1) {
    long nc = 0;
    for (int s = 0; s < S; ++s) {
      const int n = host_scene_off[s + 1] - host_scene_off[s];
      if (n > 0) nc += (n + rmax - 1) / rmax;
    }
    if (nc >= target_chunks) break;
  }
  int nc = 0, mr = 1;
  for (int s = 0; s < S; ++s) {
    const int n = host_scene_off[s + 1] - host_scene_off[s];
    if (n <= 0) continue;
    const int nck = (n + rmax - 1) / rmax, rows = (n + nck - 1) / nck;
    for (int i0 = 0; i0 < n; i0 += rows) {
      const int i1 = i0 + rows < n ? i0 + rows : n;
      if (nc >= cap) {
        sgg::set_error("%s: chunk table capacity %d exceeded", name, cap);
        return SGG_E_ARG;
      }
      chunks[4 * nc + 0] = s;
      chunks[4 * nc + 1] = i0;
      chunks[4 * nc + 2] = i1;
      chunks[4 * nc + 3] = gpw;
      if (i1 - i0 > mr) mr = i1 - i0;
      ++nc;
    }
  }
  *max_rows = mr;
  *gpw_out = gpw;
  return nc;
}

extern "C" int sgg_pool_plan_wide(const int32_t* host_scene_off, int S, int bn, int target_chunks,
                                  int32_t* chunks, int cap, int* max_rows, int* gpw_out) {
  if (!host_scene_off || !chunks || !max_rows || !gpw_out || S < 0 || cap < 0 || !wide_bn_ok(bn)) {
    sgg::set_error("sgg_pool_plan_wide: bad argument");
    return SGG_E_ARG;
  }
  return pool_plan_rows("sgg_pool_plan_wide", host_scene_off, S, wide_gpw(bn), target_chunks, chunks, cap, max_rows,
                        gpw_out);
}

extern "C" int sgg_pool_fwd_wide(const float* U, const float* pos, const float* A, const float* W2, const float* b2,
                                 const int32_t* scene_off, const int32_t* chunks, int nchunks, int max_rows, int gpw,
                                 int B, int bn, int max_n, float* out, int32_t* argmax, void* stream) {
  SGG_CHECK_ARG(U && pos && A && W2 && b2 && scene_off && chunks && out && argmax, "sgg_pool_fwd_wide: null pointer");
  SGG_CHECK_ARG(wide_bn_ok(bn), "sgg_pool_fwd_wide: bottleneck %d not built (8/16/32/48/64)", bn);
  SGG_CHECK_ARG(nchunks >= 0 && B >= 0, "sgg_pool_fwd_wide: bad sizes");
  SGG_CHECK_ARG(max_n >= 1 && max_n <= SGG_POOL_WIDE_MAX_PEDS, "sgg_pool_fwd_wide: max scene size %d outside [1, %d]",
                max_n, SGG_POOL_WIDE_MAX_PEDS);
  SGG_CHECK_ARG(max_rows >= 1 && max_rows <= 64, "sgg_pool_fwd_wide: chunk rows %d outside [1, 64]", max_rows);
  SGG_CHECK_ARG(gpw == wide_gpw(bn), "sgg_pool_fwd_wide: gpw %d is not sgg_pool_plan_wide's (%d)", gpw, wide_gpw(bn));
  hipStream_t st = (hipStream_t)stream;
  if (nchunks == 0) return 0;
  switch (bn) {
    case 8: return launch_fwd_wide<8, 2>(U, pos, A, W2, b2, scene_off, chunks, nchunks, max_rows, out, argmax, st);
    case 16: return launch_fwd_wide<16, 2>(U, pos, A, W2, b2, scene_off, chunks, nchunks, max_rows, out, argmax, st);
    case 32: return launch_fwd_wide<32, 4>(U, pos, A, W2, b2, scene_off, chunks, nchunks, max_rows, out, argmax, st);
    case 48: return launch_fwd_wide<48, 4>(U, pos, A, W2, b2, scene_off, chunks, nchunks, max_rows, out, argmax, st);
    default: return launch_fwd_wide<64, 4>(U, pos, A, W2, b2, scene_off, chunks, nchunks, max_rows, out, argmax, st);
  }
}

extern "C" int sgg_pool_bwd_wide_grid(int S, int max_n) {
  if (S < 1) return 1;
  const long long u = (long long)S * wide_bwd_jq(S, max_n);
  return (int)(u < 256 ? u : 256);
}

extern "C" int sgg_pool_bwd_wide(const float* U, const float* pos, const float* A, const float* W2, const float* out,
                                 const int32_t* argmax, const float* dout, const int32_t* scene_off, int S, int B,
                                 int bn, int max_n, float* dU, float* part, void* stream) {
  SGG_CHECK_ARG(U && pos && A && W2 && out && argmax && dout && scene_off && dU, "sgg_pool_bwd_wide: null pointer");
  SGG_CHECK_ARG(wide_bn_ok(bn), "sgg_pool_bwd_wide: bottleneck %d not built", bn);
  SGG_CHECK_ARG(max_n >= 1 && max_n <= SGG_POOL_WIDE_MAX_PEDS, "sgg_pool_bwd_wide: max scene size %d outside [1, %d]",
                max_n, SGG_POOL_WIDE_MAX_PEDS);
  SGG_CHECK_ARG(S >= 0 && B >= 0, "sgg_pool_bwd_wide: bad sizes");
  hipStream_t st = (hipStream_t)stream;
  if (S == 0) return 0;
  switch (bn) {
    case 8: return launch_bwd_wide<8>(U, pos, A, W2, out, argmax, dout, scene_off, S, max_n, dU, part, st);
    case 16: return launch_bwd_wide<16>(U, pos, A, W2, out, argmax, dout, scene_off, S, max_n, dU, part, st);
    case 32: return launch_bwd_wide<32>(U, pos, A, W2, out, argmax, dout, scene_off, S, max_n, dU, part, st);
    case 48: return launch_bwd_wide<48>(U, pos, A, W2, out, argmax, dout, scene_off, S, max_n, dU, part, st);
    default: return launch_bwd_wide<64>(U, pos, A, W2, out, argmax, dout, scene_off, S, max_n, dU, part, st);
  }
}
