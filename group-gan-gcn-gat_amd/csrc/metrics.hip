// Validation metrics of one batch in one launch (reference: scripts/train.py
// :487-568 check_accuracy with cal_l2_losses :571-581, cal_ade :584-588,
// cal_fde :591-601, sgan/utils.py relative_to_abs, losses.py gan_d_loss).
//
// Per batch the reference runs relative_to_abs (permute, cumsum, add,
// permute), two l2_loss sums, three displacement errors, three final
// displacement errors, the BCE pair and two ped counts -- about forty small
// launches -- and reads nine values back with .item().  Here a lane takes one
// ped and walks its T prediction steps: the absolute position is the running
// sum of the predicted displacements plus the start (never stored), every
// element term is formed in fp32 as the torch op forms it, and everything is
// summed in fp64:
//   lane        its ped's terms over t, in step order
//   wave        wave_sum's shuffle tree
//   workgroup   the waves in wave order -> part[workgroup][k]
//   batch       the LAST workgroup to finish (an integer ticket, as
//               sgg_adam_step's) adds the workgroups' partials in index order
//               and adds the totals into the caller's accumulator
// One order whatever the arrival order of the workgroups, no floating-point
// atomics: the same input gives the same bits.  The partials' hand-off is one
// agent-scope release before the ticket and one agent-scope acquire in the
// last arriver (plain stores and loads otherwise).
#include "bce_body.h"
#include "sgg_common.h"

namespace sgg {

constexpr int kValThreads = 256;
// a workgroup's partial sums: slots 0..7 of the accumulator, the BCE sums over
// the generated [8] and the real [9] scores, the linear [10] and non-linear
// [11] ped counts
constexpr int kValParts = SGG_VAL_SLOTS + 1;

__global__ void __launch_bounds__(kValThreads)
    val_metrics_kernel(const float* __restrict__ pred_rel, const float* __restrict__ gt,
                       const float* __restrict__ gt_rel, const float* __restrict__ start,
                       const float* __restrict__ mask, int ld, const float* __restrict__ non_linear,
                       const float* __restrict__ scores, float y_real, int T, int B, double* acc, double* part,
                       unsigned* ticket) {
#pragma clang fp contract(off)   // every fp32 term rounds where the torch op it replaces rounds
  __shared__ double red[kValThreads / 64][kValParts];
  __shared__ int last;
  const long long p = (long long)blockIdx.x * kValThreads + threadIdx.x;
  const bool live = p < B;
  const size_t q = live ? (size_t)p : (size_t)B - 1;   // (a lane past the end reads the last ped and counts for 0)
  const size_t step = 2 * (size_t)B;
  const float sx = start[2 * q], sy = start[2 * q + 1];
  const float nl = non_linear[q];
  const float* mrow = mask + q * (size_t)ld;
  float cx = 0.f, cy = 0.f, fd = 0.f;
  double l2a = 0.0, l2r = 0.0, ade = 0.0;
#pragma unroll 4
  for (int t = 0; t < T; ++t) {
    const size_t o = (size_t)t * step + 2 * q;
    const float rx = pred_rel[o], ry = pred_rel[o + 1];
    const float gx = gt[o], gy = gt[o + 1];
    const float hx = gt_rel[o], hy = gt_rel[o + 1];
    const float m = mrow[t];
    cx += rx;   // relative_to_abs: cumsum over the steps, then + start
    cy += ry;
    const float dx = gx - (cx + sx), dy = gy - (cy + sy);
    const float ex = dx * dx, ey = dy * dy;
    l2a += (double)(m * ex) + (double)(m * ey);
    fd = sqrtf(ex + ey);
    ade += (double)fd;
    const float ux = hx - rx, uy = hy - ry;
    l2r += (double)(m * (ux * ux)) + (double)(m * (uy * uy));
  }
  const float lin = 1.f - nl;
  double v[kValParts];
  v[0] = l2a;
  v[1] = l2r;
  v[2] = ade;
  v[3] = ade * (double)lin;
  v[4] = ade * (double)nl;
  v[5] = (double)fd;
  v[6] = (double)(fd * lin);
  v[7] = (double)(fd * nl);
  v[8] = scores ? (double)bce_term(scores[q], 0.f) : 0.0;
  v[9] = scores ? (double)bce_term(scores[(size_t)B + q], y_real) : 0.0;
  v[10] = (double)lin;
  v[11] = (double)nl;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < kValParts; ++k) {
    const double s = wave_sum(live ? v[k] : 0.0);
    if (lane == 0) red[wave][k] = s;
  }
  __syncthreads();
  if (threadIdx.x < kValParts) {
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < kValThreads / 64; ++w) s += red[w][threadIdx.x];
    part[(size_t)blockIdx.x * kValParts + threadIdx.x] = s;
  }
  // publish the partials, take a ticket; the last arriver reads them all
  __asm__ volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    __asm__ volatile("s_waitcnt vmcnt(0)" ::: "memory");
    last = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1;
    if (last) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      __asm__ volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
  }
  __syncthreads();
  if (!last) return;
  if (threadIdx.x < kValParts) {
    double s = 0.0;
    for (unsigned b = 0; b < gridDim.x; ++b) s += part[(size_t)b * kValParts + threadIdx.x];
    red[0][threadIdx.x] = s;
  }
  __syncthreads();
  if (threadIdx.x < 8) acc[threadIdx.x] += red[0][threadIdx.x];
  // gan_d_loss: bce_loss(real, y_real) + bce_loss(fake, 0), each a mean over B
  if (threadIdx.x == 8 && scores) acc[8] += red[0][9] / (double)B + red[0][8] / (double)B;
  if (threadIdx.x == 9 || threadIdx.x == 10) acc[threadIdx.x] += red[0][threadIdx.x + 1];
  if (threadIdx.x == 0) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__host__ static long long val_blocks(int B) { return ((long long)B + kValThreads - 1) / kValThreads; }

}  // namespace sgg

using namespace sgg;

// work: the ticket word and a pad word, then kValParts doubles per workgroup
extern "C" size_t sgg_val_metrics_work_floats(int B) {
  return B < 1 ? 0 : 2 + 2 * (size_t)kValParts * (size_t)val_blocks(B);
}

extern "C" int sgg_val_metrics(const float* pred_rel, const float* gt, const float* gt_rel, const float* start,
                               const float* mask, int ld, const float* non_linear, const float* scores,
                               float y_real, int T, int B, double* acc, float* work, void* stream) {
  SGG_CHECK_ARG(pred_rel && gt && gt_rel && start && mask && non_linear && acc && work,
                "sgg_val_metrics: null pointer");
  SGG_CHECK_ARG(B >= 1 && T >= 1, "sgg_val_metrics: bad sizes T=%d B=%d", T, B);
  SGG_CHECK_ARG(ld >= T, "sgg_val_metrics: mask row stride %d below T=%d", ld, T);
  SGG_CHECK_ARG(((uintptr_t)acc & 7) == 0 && ((uintptr_t)work & 7) == 0, "sgg_val_metrics: acc / work not 8-byte aligned");
  unsigned* ticket = reinterpret_cast<unsigned*>(work);
  double* part = reinterpret_cast<double*>(work + 2);
  hipLaunchKernelGGL(val_metrics_kernel, dim3((unsigned)val_blocks(B)), dim3(kValThreads), 0, (hipStream_t)stream,
                     pred_rel, gt, gt_rel, start, mask, ld, non_linear, scores, y_real, T, B, acc, part, ticket);
  SGG_RETURN_LAUNCH("sgg_val_metrics");
}
