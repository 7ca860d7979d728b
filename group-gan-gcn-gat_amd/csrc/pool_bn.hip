// Social pooling at any bottleneck_dim 1 .. SGG_POOL_BN_MAX: the 512 -> bn
// layer cut into column tiles of <= 64 columns, bn a runtime argument.  Same
// operands, outputs and argmax contract as pool_wide.hip, whose pair-space
// tiling (j tiles forward, (scene, j range) units x i tiles backward) is kept;
// nothing in registers or LDS grows with bn.
#include "sgg_common.h"
#include "pool_common.h"
#include "pool_tiled_fwd.h"

namespace sgg {

// ---- forward ------------------------------------------------------------------
// pool_fwd_wide_kernel<64, 4>'s body (pool_tiled_fwd.h, shared code) with the column tile as grid
// dimension y: the workgroup (x, y) walks x's row chunks against columns [64 y, 64 y + 64) of
// W2 / b2 / out / argmax, all addressed with the runtime row stride bn.  A pair's value in a column
// is the wide kernel's (same hidden FMA chain, same k order through v_mfma_f32_16x16x4_f32, bias,
// ReLU; an MFMA column does not see its neighbours).  Columns >= bn of the last tile: W2 rows read
// as 0, nothing max-ed or stored.  The hidden units are recomputed per column tile (2 FMA + max
// against 2 x 64 MFMA flop per tile), which keeps the keys in LDS at rows x 64 and gives every tile
// its own workgroups.
constexpr int kBT = 64;            // columns per tile
constexpr int kBGPW = 4;           // pair groups per wave
constexpr int kHid = kHidden;

__global__ void __launch_bounds__(256) pool_fwd_bn_kernel(
    const float* __restrict__ U, const float* __restrict__ pos, const float* __restrict__ A,
    const float* __restrict__ W2 /* bn x 512 */, const float* __restrict__ b2,
    const int32_t* __restrict__ scene_off, const int4* __restrict__ chunks, int nch, int bn,
    float* __restrict__ out, int32_t* __restrict__ argmax) {
  // (grid.y = ceil(bn / 64): every tile has at least one live column)
  pool_fwd_tiled_body<kBT, kBGPW, true>(U, pos, A, W2, b2, scene_off, chunks, nch, out, argmax,
                                        (int)blockIdx.y * kBT, bn);
}

// ---- backward -----------------------------------------------------------------
// Two launches on the one stream.  Both walk pool_bwd_wide_kernel's work
// units -- (scene, j range of <= kBJR peds), the scene's i in tiles of 64
// ascending, per tile the (j, c) masks over i rebuilt by LDS atomic OR, thread
// k = hidden unit k -- and both recompute a pair's pre-activation the same way.
//
// pool_bwd_bn_du_kernel: dU and dA.  One unit per workgroup trip as in the wide
// kernel; inside a unit the column tiles run ascending, W2's 64 columns of the
// tile in registers, dU[j, k] carried across tiles in the thread's own LDS
// column.  Order of every dU sum: column tiles ascending, then i tiles
// ascending, then columns, then i ascending -- with one tile, the wide
// kernel's order and chain, so dU is bitwise its dU.  The workgroup's dA
// partial goes to its own 1024 floats after the slab.
//
// pool_bwd_bn_dw_kernel: dW2 and db2, which are sums per column.  Workgroup
// (g, r) owns the kBCG columns from kBCG g and the units r, r + kBRows, ..; it
// keeps dW2[c][k] of its columns in registers over all its units and writes
// them into row r of the slab -- so the slab has kBRows rows whatever the grid,
// and no workgroup holds more than kBCG columns.  The g = 0 workgroup of row r
// also folds the first launch's dA partials r, r + kBRows, .. (ascending) into
// the row's dA columns.  No floating-point atomics anywhere.
constexpr int kBJR = 16;     // peds of a j range (pool_wide.hip kWideJR)
constexpr int kBCG = 16;     // columns of a dW2 workgroup
constexpr int kBRows = 8;    // rows of the parameter-gradient slab

template <bool WGRAD>
__global__ void __launch_bounds__(512) pool_bwd_bn_du_kernel(
    const float* __restrict__ U, const float* __restrict__ pos, const float* __restrict__ A,
    const float* __restrict__ W2 /* bn x 512 */, const float* __restrict__ out,
    const int32_t* __restrict__ argmax, const float* __restrict__ dout, const int32_t* __restrict__ scene_off,
    int S, int jq, int bn, float* __restrict__ dU, float* __restrict__ dAp /* grid x 1024 */) {
  constexpr int BN = kBT;
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
            const float g = ov > 0.f ? dv : 0.f;
            gs[e] = g;
            if (g != 0.f && jl >= 0 && jl < nr) atomicOr(&msk[jl * BN + c], 1ull << i);
          }
        }
        __syncthreads();
        for (int r = 0; r < nr; ++r) {
          const float u = Us[r * kHid + k];
          const float2 pj = ps[j0 + r];
          float du = dUs[r * kHid + k];
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
            auto entry = [&](float g, float2 pi) {
              const float rx = pj.x - pi.x, ry = pj.y - pi.y;
              const float pre = fmaf(a1, ry, fmaf(a0, rx, u));
              const float gm = pre > 0.f ? g : 0.f;
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
              entry(g, pi);
              if (two) entry(g2, pi2);
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

__global__ void __launch_bounds__(512) pool_bwd_bn_dw_kernel(
    const float* __restrict__ U, const float* __restrict__ pos, const float* __restrict__ A,
    const float* __restrict__ out, const int32_t* __restrict__ argmax, const float* __restrict__ dout,
    const int32_t* __restrict__ scene_off, int S, int jq, int bn, const float* __restrict__ dAp, int ndA,
    float* __restrict__ part /* kBRows x (bn*512 + 1024 + bn) */) {
  constexpr int CG = kBCG;
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
          g = ov > 0.f ? dv : 0.f;
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
            dw2[c] = fmaf(gm, pre, dw2[c]);
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

// j ranges per scene (pool_wide.hip wide_bwd_jq): a range fits the LDS rows,
// more ranges while S x jq stays within one round of the chip
static int bn_bwd_jq(int S, int max_n) {
  if (S < 1 || max_n < 1) return 1;
  int jq = (max_n + kBJR - 1) / kBJR;
  const int fill = 256 / S;
  if (fill > jq) jq = fill < max_n ? fill : max_n;
  return jq < 1 ? 1 : jq;
}

static long long bn_slab_cols(int bn) { return (long long)bn * kHid + 2 * kHid + bn; }

// workgroups of the dU launch = dA partials behind the slab: one per unit up
// to 256, and no more than fit in another kBRows slab rows (the workspace
// stays within 2 kBRows = 16 rows at every bn; binds below bn = 64 only)
static int bn_bwd_du_grid(int S, int bn, int max_n) {
  if (S < 1) return 1;
  long long g = (long long)S * bn_bwd_jq(S, max_n);
  if (g > 256) g = 256;
  const long long fit = (long long)kBRows * bn_slab_cols(bn) / (2 * kHid);
  if (g > fit) g = fit;
  return (int)(g < 1 ? 1 : g);
}

}  // namespace sgg

using namespace sgg;

static bool bn_sizes_ok(const char* name, int bn, int max_n) {
  if (bn < 1 || bn > SGG_POOL_BN_MAX) {
    sgg::set_error("%s: bottleneck %d outside [1, %d]", name, bn, SGG_POOL_BN_MAX);
    return false;
  }
  if (max_n < 1 || max_n > SGG_POOL_WIDE_MAX_PEDS) {
    sgg::set_error("%s: max scene size %d outside [1, %d]", name, max_n, SGG_POOL_WIDE_MAX_PEDS);
    return false;
  }
  return true;
}

extern "C" int sgg_pool_plan_bn(const int32_t* host_scene_off, int S, int bn, int target_chunks, int32_t* chunks,
                                int cap, int* max_rows, int* gpw_out) {
  SGG_CHECK_ARG(host_scene_off && chunks && max_rows && gpw_out, "sgg_pool_plan_bn: null pointer");
  SGG_CHECK_ARG(S >= 0 && cap >= 0, "sgg_pool_plan_bn: bad sizes");
  SGG_CHECK_ARG(bn >= 1 && bn <= SGG_POOL_BN_MAX, "sgg_pool_plan_bn: bottleneck %d outside [1, %d]", bn,
                SGG_POOL_BN_MAX);
  return pool_plan_rows("sgg_pool_plan_bn", host_scene_off, S, kBGPW, target_chunks, chunks, cap, max_rows, gpw_out);
}

extern "C" int sgg_pool_fwd_bn(const float* U, const float* pos, const float* A, const float* W2, const float* b2,
                               const int32_t* scene_off, const int32_t* chunks, int nchunks, int max_rows, int gpw,
                               int B, int bn, int max_n, float* out, int32_t* argmax, void* stream) {
  SGG_CHECK_ARG(U && pos && A && W2 && b2 && scene_off && chunks && out && argmax, "sgg_pool_fwd_bn: null pointer");
  if (!bn_sizes_ok("sgg_pool_fwd_bn", bn, max_n)) return SGG_E_ARG;
  SGG_CHECK_ARG(nchunks >= 0 && B >= 0, "sgg_pool_fwd_bn: bad sizes");
  SGG_CHECK_ARG(max_rows >= 1 && max_rows <= 64, "sgg_pool_fwd_bn: chunk rows %d outside [1, 64]", max_rows);
  SGG_CHECK_ARG(gpw == kBGPW, "sgg_pool_fwd_bn: gpw %d is not sgg_pool_plan_bn's (%d)", gpw, kBGPW);
  if (nchunks == 0) return 0;
  // x: a multiple of 8 workgroups (XCD-aware order), x * y at most about four rounds of the chip
  const int nct = (bn + kBT - 1) / kBT;
  int grid = (nchunks + 7) & ~7;
  int cap = (4 * device_cus() / nct + 7) & ~7;
  if (cap < 8) cap = 8;
  if (grid > cap) grid = cap;
  hipLaunchKernelGGL(pool_fwd_bn_kernel, dim3(grid, nct), dim3(256), pool_fwd_tiled_lds<kBT>(max_rows), (hipStream_t)stream, U, pos,
                     A, W2, b2, scene_off, reinterpret_cast<const int4*>(chunks), nchunks, bn, out, argmax);
  SGG_RETURN_LAUNCH("sgg_pool_fwd_bn");
}

extern "C" int sgg_pool_bwd_bn_grid(int S, int bn, int max_n) {
  SGG_CHECK_ARG(S >= 0, "sgg_pool_bwd_bn_grid: bad sizes");
  if (!bn_sizes_ok("sgg_pool_bwd_bn_grid", bn, max_n)) return SGG_E_ARG;
  return kBRows;
}

extern "C" long long sgg_pool_bwd_bn_ws_floats(int S, int B, int bn, int max_n) {
  if (S < 0 || B < 0) {
    sgg::set_error("sgg_pool_bwd_bn_ws_floats: bad sizes");
    return SGG_E_ARG;
  }
  if (!bn_sizes_ok("sgg_pool_bwd_bn_ws_floats", bn, max_n)) return SGG_E_ARG;
  return kBRows * bn_slab_cols(bn) + (long long)bn_bwd_du_grid(S, bn, max_n) * 2 * kHid;
}

extern "C" int sgg_pool_bwd_bn(const float* U, const float* pos, const float* A, const float* W2, const float* out,
                               const int32_t* argmax, const float* dout, const int32_t* scene_off, int S, int B, int bn,
                               int max_n, float* dU, float* part, size_t part_floats, void* stream) {
  SGG_CHECK_ARG(U && pos && A && W2 && out && argmax && dout && scene_off && dU, "sgg_pool_bwd_bn: null pointer");
  if (!bn_sizes_ok("sgg_pool_bwd_bn", bn, max_n)) return SGG_E_ARG;
  SGG_CHECK_ARG(S >= 0 && B >= 0, "sgg_pool_bwd_bn: bad sizes");
  const long long need = sgg_pool_bwd_bn_ws_floats(S, B, bn, max_n);
  SGG_CHECK_ARG(!part || (long long)part_floats >= need,
                "sgg_pool_bwd_bn: workspace of %zu floats, sgg_pool_bwd_bn_ws_floats asks for %lld", part_floats, need);
  hipStream_t st = (hipStream_t)stream;
  if (S == 0) return 0;
  const int jq = bn_bwd_jq(S, max_n);
  const int grid = bn_bwd_du_grid(S, bn, max_n);
  float* dAp = part ? part + (size_t)kBRows * bn_slab_cols(bn) : nullptr;
  if (part)
    hipLaunchKernelGGL(pool_bwd_bn_du_kernel<true>, dim3(grid), dim3(512), 0, st, U, pos, A, W2, out, argmax, dout,
                       scene_off, S, jq, bn, dU, dAp);
  else
    hipLaunchKernelGGL(pool_bwd_bn_du_kernel<false>, dim3(grid), dim3(512), 0, st, U, pos, A, W2, out, argmax, dout,
                       scene_off, S, jq, bn, dU, dAp);
  {
    hipError_t e_ = hipGetLastError();
    if (e_ != hipSuccess) {
      sgg::set_error("sgg_pool_bwd_bn: launch failed: %s", hipGetErrorString(e_));
      return (int)e_;
    }
  }
  if (!part) return 0;
  hipLaunchKernelGGL(pool_bwd_bn_dw_kernel, dim3((bn + kBCG - 1) / kBCG, kBRows), dim3(512), 0, st, U, pos, A, out,
                     argmax, dout, scene_off, S, jq, bn, dAp, grid, part);
  SGG_RETURN_LAUNCH("sgg_pool_bwd_bn");
}
