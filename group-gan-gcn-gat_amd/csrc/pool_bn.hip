// Social pooling at any bottleneck_dim 1 .. SGG_POOL_BN_MAX: the 512 -> bn
// layer cut into column tiles of <= 64 columns, bn a runtime argument.  Same
// operands, outputs and argmax contract as pool_wide.hip, whose pair-space
// tiling (j tiles forward, (scene, j range) units x i tiles backward) is kept;
// nothing in registers or LDS grows with bn.
#include "sgg_common.h"
#include "pool_common.h"
#include "pool_tiled_fwd.h"
#include "pool_drop.h"

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

// The dropout form (sgg_pool_fwd_bn_drop): the same body with the two scaled masks of pool_drop.h -- the
// hidden value m1 * relu(u + a . rel), the epilogue value m2 * relu(acc + b2) -- both functions of
// (i, j, column) alone, so every column tile forms the same hidden units.
__global__ void __launch_bounds__(256) pool_fwd_bn_drop_kernel(
    const float* __restrict__ U, const float* __restrict__ pos, const float* __restrict__ A,
    const float* __restrict__ W2 /* bn x 512 */, const float* __restrict__ b2,
    const int32_t* __restrict__ scene_off, const int4* __restrict__ chunks, int nch, int bn,
    float* __restrict__ out, int32_t* __restrict__ argmax, DropArgs drop) {
  pool_fwd_tiled_body<kBT, kBGPW, true, true>(U, pos, A, W2, b2, scene_off, chunks, nch, out, argmax,
                                              (int)blockIdx.y * kBT, bn, drop);
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

// pool_bwd_bn_du_kernel<WGRAD> / pool_bwd_bn_dw_kernel and their dropout forms: one text
// (pool_bn_bwd.h) compiled twice
#define SGG_POOL_DROP 0
#include "pool_bn_bwd.h"
#undef SGG_POOL_DROP
#define SGG_POOL_DROP 1
#include "pool_bn_bwd.h"
#undef SGG_POOL_DROP

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

// sgg_pool_fwd_bn (drop == NULL) and sgg_pool_fwd_bn_drop: the same checks, grid and LDS
static int fwd_bn(const char* name, const float* U, const float* pos, const float* A, const float* W2, const float* b2,
                  const int32_t* scene_off, const int32_t* chunks, int nchunks, int max_rows, int gpw, int B, int bn,
                  int max_n, float* out, int32_t* argmax, const DropArgs* drop, void* stream) {
  SGG_CHECK_ARG(U && pos && A && W2 && b2 && scene_off && chunks && out && argmax, "%s: null pointer", name);
  if (!bn_sizes_ok(name, bn, max_n)) return SGG_E_ARG;
  SGG_CHECK_ARG(nchunks >= 0 && B >= 0, "%s: bad sizes", name);
  SGG_CHECK_ARG(max_rows >= 1 && max_rows <= 64, "%s: chunk rows %d outside [1, 64]", name, max_rows);
  SGG_CHECK_ARG(gpw == kBGPW, "%s: gpw %d is not sgg_pool_plan_bn's (%d)", name, gpw, kBGPW);
  if (nchunks == 0) return 0;
  // x: a multiple of 8 workgroups (XCD-aware order), x * y at most about four rounds of the chip
  const int nct = (bn + kBT - 1) / kBT;
  int grid = (nchunks + 7) & ~7;
  int cap = (4 * device_cus() / nct + 7) & ~7;
  if (cap < 8) cap = 8;
  if (grid > cap) grid = cap;
  if (drop)
    hipLaunchKernelGGL(pool_fwd_bn_drop_kernel, dim3(grid, nct), dim3(256), pool_fwd_tiled_lds<kBT>(max_rows),
                       (hipStream_t)stream, U, pos, A, W2, b2, scene_off, reinterpret_cast<const int4*>(chunks), nchunks,
                       bn, out, argmax, *drop);
  else
    hipLaunchKernelGGL(pool_fwd_bn_kernel, dim3(grid, nct), dim3(256), pool_fwd_tiled_lds<kBT>(max_rows), (hipStream_t)stream, U, pos,
                       A, W2, b2, scene_off, reinterpret_cast<const int4*>(chunks), nchunks, bn, out, argmax);
  SGG_RETURN_LAUNCH(name);
}

extern "C" int sgg_pool_fwd_bn(const float* U, const float* pos, const float* A, const float* W2, const float* b2,
                               const int32_t* scene_off, const int32_t* chunks, int nchunks, int max_rows, int gpw,
                               int B, int bn, int max_n, float* out, int32_t* argmax, void* stream) {
  return fwd_bn("sgg_pool_fwd_bn", U, pos, A, W2, b2, scene_off, chunks, nchunks, max_rows, gpw, B, bn, max_n, out,
                argmax, nullptr, stream);
}

extern "C" int sgg_pool_fwd_bn_drop(const float* U, const float* pos, const float* A, const float* W2, const float* b2,
                                    const int32_t* scene_off, const int32_t* chunks, int nchunks, int max_rows,
                                    int gpw, int B, int bn, int max_n, float* out, int32_t* argmax, float p,
                                    unsigned long long seed, unsigned offset, const unsigned long long* rng_dev,
                                    void* stream) {
  DropArgs d;
  if (!pool_drop_args("sgg_pool_fwd_bn_drop", p, seed, offset, rng_dev, &d)) return SGG_E_ARG;
  return fwd_bn("sgg_pool_fwd_bn_drop", U, pos, A, W2, b2, scene_off, chunks, nchunks, max_rows, gpw, B, bn, max_n, out,
                argmax, &d, stream);
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

// sgg_pool_bwd_bn (drop == NULL) and sgg_pool_bwd_bn_drop: the same checks, grids and workspace
static int bwd_bn(const char* name, const float* U, const float* pos, const float* A, const float* W2, const float* out,
                  const int32_t* argmax, const float* dout, const int32_t* scene_off, int S, int B, int bn, int max_n,
                  float* dU, float* part, size_t part_floats, const DropArgs* drop, void* stream) {
  SGG_CHECK_ARG(U && pos && A && W2 && out && argmax && dout && scene_off && dU, "%s: null pointer", name);
  if (!bn_sizes_ok(name, bn, max_n)) return SGG_E_ARG;
  SGG_CHECK_ARG(S >= 0 && B >= 0, "%s: bad sizes", name);
  const long long need = sgg_pool_bwd_bn_ws_floats(S, B, bn, max_n);
  SGG_CHECK_ARG(!part || (long long)part_floats >= need,
                "%s: workspace of %zu floats, sgg_pool_bwd_bn_ws_floats asks for %lld", name, part_floats, need);
  hipStream_t st = (hipStream_t)stream;
  if (S == 0) return 0;
  const int jq = bn_bwd_jq(S, max_n);
  const int grid = bn_bwd_du_grid(S, bn, max_n);
  float* dAp = part ? part + (size_t)kBRows * bn_slab_cols(bn) : nullptr;
  if (drop && part)
    hipLaunchKernelGGL(pool_bwd_bn_du_drop_kernel<true>, dim3(grid), dim3(512), 0, st, U, pos, A, W2, out, argmax, dout,
                       scene_off, S, jq, bn, dU, dAp, *drop);
  else if (drop)
    hipLaunchKernelGGL(pool_bwd_bn_du_drop_kernel<false>, dim3(grid), dim3(512), 0, st, U, pos, A, W2, out, argmax,
                       dout, scene_off, S, jq, bn, dU, dAp, *drop);
  else if (part)
    hipLaunchKernelGGL(pool_bwd_bn_du_kernel<true>, dim3(grid), dim3(512), 0, st, U, pos, A, W2, out, argmax, dout,
                       scene_off, S, jq, bn, dU, dAp);
  else
    hipLaunchKernelGGL(pool_bwd_bn_du_kernel<false>, dim3(grid), dim3(512), 0, st, U, pos, A, W2, out, argmax, dout,
                       scene_off, S, jq, bn, dU, dAp);
  {
    hipError_t e_ = hipGetLastError();
    if (e_ != hipSuccess) {
      sgg::set_error("%s: launch failed: %s", name, hipGetErrorString(e_));
      return (int)e_;
    }
  }
  if (!part) return 0;
  if (drop)
    hipLaunchKernelGGL(pool_bwd_bn_dw_drop_kernel, dim3((bn + kBCG - 1) / kBCG, kBRows), dim3(512), 0, st, U, pos, A,
                       out, argmax, dout, scene_off, S, jq, bn, dAp, grid, part, *drop);
  else
    hipLaunchKernelGGL(pool_bwd_bn_dw_kernel, dim3((bn + kBCG - 1) / kBCG, kBRows), dim3(512), 0, st, U, pos, A, out,
                       argmax, dout, scene_off, S, jq, bn, dAp, grid, part);
  SGG_RETURN_LAUNCH(name);
}

extern "C" int sgg_pool_bwd_bn(const float* U, const float* pos, const float* A, const float* W2, const float* out,
                               const int32_t* argmax, const float* dout, const int32_t* scene_off, int S, int B, int bn,
                               int max_n, float* dU, float* part, size_t part_floats, void* stream) {
  return bwd_bn("sgg_pool_bwd_bn", U, pos, A, W2, out, argmax, dout, scene_off, S, B, bn, max_n, dU, part, part_floats,
                nullptr, stream);
}

extern "C" int sgg_pool_bwd_bn_drop(const float* U, const float* pos, const float* A, const float* W2,
                                    const float* out, const int32_t* argmax, const float* dout,
                                    const int32_t* scene_off, int S, int B, int bn, int max_n, float* dU, float* part,
                                    size_t part_floats, float p, unsigned long long seed, unsigned offset,
                                    const unsigned long long* rng_dev, void* stream) {
  DropArgs d;
  if (!pool_drop_args("sgg_pool_bwd_bn_drop", p, seed, offset, rng_dev, &d)) return SGG_E_ARG;
  return bwd_bn("sgg_pool_bwd_bn_drop", U, pos, A, W2, out, argmax, dout, scene_off, S, B, bn, max_n, dU, part,
                part_floats, &d, stream);
}
