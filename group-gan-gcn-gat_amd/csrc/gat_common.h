// Shared by the attention kernels of gat.hip (a segment LDS-resident) and
// gat_wide.hip (the pair space of a segment tiled).
#pragma once
#include "sgg_common.h"

namespace sgg {

constexpr int kGatThreads = 256;
constexpr int kGatWaves = kGatThreads / 64;

__device__ __forceinline__ float lrelu(float x, float alpha) { return x > 0.f ? x : alpha * x; }

// LDS row stride of a staged node tile: F rounded up to the 4-feature MFMA
// k-step (the pad columns hold zeros), odd
__host__ __device__ __forceinline__ int gat_fs(int F) { return ((F + 3) & ~3) | 1; }
__host__ __device__ __forceinline__ int gat_r16(int n) { return (n + 15) & ~15; }

// A rows x cols block into LDS with 16 loads in flight per thread (a loop
// of one load and one store per element waits a memory latency per
// element): ld(r, c) is called with indices clamped into [0, nv) x [0, cv)
// and its value masked to zero outside; st(r, c, v) stores it
template <typename Ld, typename St>
__device__ __forceinline__ void stage_block(int rows, int cols, int nv, int cv, Ld ld, St st) {
  constexpr int kU = 16;
  const int total = rows * cols;
  const int dq = kGatThreads / cols, dr = kGatThreads - dq * cols;   // one step of kGatThreads elements
  for (int base = 0; base < total; base += kU * kGatThreads) {
    const int e0 = base + (int)threadIdx.x;
    const int r0 = e0 / cols, c0 = e0 - r0 * cols;
    float v[kU];
    int r = r0, c = c0;
#pragma unroll
    for (int u = 0; u < kU; ++u) {   // (slots past the block load a clamped element: no branch)
      v[u] = keep_if(ld(min(r, nv - 1), min(c, cv - 1)), r < nv && c < cv);
      r += dq;
      c += dr;
      if (c >= cols) {
        c -= cols;
        ++r;
      }
    }
    r = r0;
    c = c0;
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      if (e0 + u * kGatThreads < total) st(r, c, v[u]);
      r += dq;
      c += dr;
      if (c >= cols) {
        c -= cols;
        ++r;
      }
    }
  }
}

// s_i = Wh_i . a_src, t_i = Wh_i . a_dst (a_s / a_d: LDS copies) and the
// labels of rows [0, nr) (Ws rows >= n are zero): each row's dot products
// split over 256 / nr lanes (a shuffle tree joins them); the caller barriers.
// nseg_r (gat_wide.hip: Ws holds one tile of a segment of nseg_r padded
// rows): the rows that set the lane split, so a tile's scores are summed as
// the whole segment's would be
__device__ __forceinline__ void gat_scores(const float* Ws, int Fs, const float* a_s, const float* a_d, int F,
                                           const float* labels, int mode, int o, int n, int nr, float* ss, float* ts,
                                           float* lab, const float* Ds = nullptr, float* rsum = nullptr,
                                           int nseg_r = 0) {
  const int nsp = nseg_r ? nseg_r : nr;
  int sp = 1;   // lanes per row: a power of 2 (groups of aligned lanes)
  while (sp < 16 && 2 * sp * nsp <= kGatThreads) sp *= 2;
  const int part = threadIdx.x & (sp - 1);
  for (int r = threadIdx.x / sp; r < nr; r += kGatThreads / sp) {
    // (fp64: the products of two floats are exact, so the scores are the
    // rounded exact dot products whatever the lane split)
    double s = 0.0, t = 0.0;
    float sd = 0.f;
    for (int f = part; f < F; f += sp) {
      const double w = Ws[r * Fs + f];
      s = fma(w, (double)a_s[f], s);
      t = fma(w, (double)a_d[f], t);
      if (Ds) sd += Ds[r * Fs + f];
    }
    for (int o2 = 1; o2 < sp; o2 <<= 1) {
      s += __shfl_xor(s, o2);
      t += __shfl_xor(t, o2);
      sd += __shfl_xor(sd, o2);
    }
    if (part == 0) {
      ss[r] = (float)s;
      ts[r] = (float)t;
      if (rsum) rsum[r] = sd;
      lab[r] = (mode == 0 && r < n) ? labels[o + r] : 0.f;
    }
  }
}

// Epilogue (0 identity, 1 ELU, 2 log_softmax(ELU(.)) over F) and stores of a
// 16-row block of aggregates in the MFMA C layout: hv[ct][v] = row I0 + 4 q +
// v (segment-local, valid below n), feature 16 ct + r16.  A macro over the
// caller's hv, nct, F, epi, n, o, HF, c0, r16, q, hp, y, ldy: as a function
// taking hv by reference it compiles gat_fwd_kernel / gat_layer_fwd_kernel to
// other instruction streams than the text in place does.
#define SGG_GAT_EPILOGUE_STORE(I0)                                              \
  {                                                                             \
    float lse[4] = {0.f, 0.f, 0.f, 0.f};                                        \
    if (epi == 2) {                                                             \
    _Pragma("unroll")                                                           \
      for (int v = 0; v < 4; ++v) {                                             \
        float zm = -INFINITY;                                                   \
    _Pragma("unroll")                                                           \
        for (int ct = 0; ct < 8; ++ct)                                          \
          if (ct < nct && 16 * ct + r16 < F) zm = fmaxf(zm, elu(hv[ct][v]));    \
    _Pragma("unroll")                                                           \
        for (int o2 = 1; o2 < 16; o2 <<= 1) zm = fmaxf(zm, __shfl_xor(zm, o2)); \
        float se = 0.f;                                                         \
    _Pragma("unroll")                                                           \
        for (int ct = 0; ct < 8; ++ct)                                          \
          if (ct < nct && 16 * ct + r16 < F) se += expf(elu(hv[ct][v]) - zm);   \
    _Pragma("unroll")                                                           \
        for (int o2 = 1; o2 < 16; o2 <<= 1) se += __shfl_xor(se, o2);           \
        lse[v] = zm + logf(se);                                                 \
      }                                                                         \
    }                                                                           \
    _Pragma("unroll")                                                           \
    for (int ct = 0; ct < 8; ++ct) {                                            \
      const int f = 16 * ct + r16;                                              \
      if (ct < nct && f < F) {                                                  \
    _Pragma("unroll")                                                           \
        for (int v = 0; v < 4; ++v) {                                           \
          const int io = (I0) + 4 * q + v;                                      \
          if (io < n) {                                                         \
            const float h = hv[ct][v];                                          \
            const float z = epi ? elu(h) : h;                                   \
            if (epi) hp[(size_t)(o + io) * HF + c0 + f] = h;                    \
            y[(size_t)(o + io) * ldy + c0 + f] = epi == 2 ? z - lse[v] : z;     \
          }                                                                     \
        }                                                                       \
      }                                                                         \
    }                                                                           \
  }

// rows past the last segment (zero-padded group buffers): zero outputs
// (blk / nblk: this workgroup's index among the nblk serving the rows)
__device__ __forceinline__ void gat_zero_pad_rows(int tot, int nrows, int HF, float* y, int ldy, float* hp,
                                                  int blk = -1, int nblk = 0) {
  if (blk < 0) {
    blk = blockIdx.x;
    nblk = gridDim.x;
  }
  for (size_t e = (size_t)tot * HF + (size_t)blk * kGatThreads + threadIdx.x; e < (size_t)nrows * HF;
       e += (size_t)nblk * kGatThreads) {
    const size_t r = e / HF, c = e - r * HF;
    y[r * ldy + c] = 0.f;
    if (hp) hp[e] = 0.f;
  }
}

// gat.hip: da_src / da_dst (heads x F each) and dbias (F, may be NULL) from
// `rows` slab rows of per-head partials -- pda rows x heads x 2F floats, pdb
// rows x heads x F doubles -- in one fixed-order launch; internal
__attribute__((visibility("hidden"))) void gat_param_reduce(const float* pda, const double* pdb, int rows, int heads,
                                                            int F, float* da_src, float* da_dst, float* dbias,
                                                            hipStream_t st);

}  // namespace sgg
